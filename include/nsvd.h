/*
 * nsvd.h - C ABI of libnsvd_hip.so: the MI355X (gfx950) NestedLoRA / NeuralSVD PDE training step.
 *
 * This is the drop-in boundary for ONE path of jongharyu/neural-svd (all citations are paths in
 * that repository):
 *
 *     loss, aux = method.compute_loss_operator(operator, x, importance)   methods/nestedlora.py:254-267
 *     loss.backward(); optimizer.step(); ema.update()                     examples/operator/__init__.py:55-74
 *     compute_spectrum_evd(...)                                           methods/spectrum.py:29-102
 *
 * The reference has no FFI (it is pure Python on torch eager ops); the entry points below are the
 * functions a maintainer would bind (ctypes stub in INTEGRATION.md) to replace the torch op
 * sequences cited per function.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous float32 unless it says "host";
 *   - the caller owns every buffer, including the workspace (size: nsvd_workspace_bytes);
 *     nothing here allocates, frees or synchronises;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*), is safe to capture in
 *     a HIP graph (no allocation, no synchronisation, no host read-back: tests/test_graph_gpu.py captures and
 *     replays the training step), and keeps no global mutable state (re-entrant across streams / devices).
 *     The scalars that change from step to step (scheduled learning rate, EMA decay, sampler counter) are kernel
 *     ARGUMENTS in the plain entry points - a captured step replays them frozen - and live in device memory
 *     when the caller passes a nsvd_step_state (below): that form replays a moving schedule;
 *   - return value: 0 on success, negative on error (-(int)hipError_t for HIP failures,
 *     NSVD_EINVAL / NSVD_EUNSUPPORTED for argument errors); no C++ exception crosses the ABI.
 *
 * Tensor layouts (B = batch rows, D = space dims, E = 1 + 2D stencil points, R = E*B stencil
 * rows ordered [x, x+eps e_0, x-eps e_0, x+eps e_1, ...] x B, L = eigenfunctions/heads,
 * m = Fourier mapping size, F = 2m features, h_i = width of layer i, h_last = 1):
 *     x        (B, D)           row-major
 *     fourier_B(D, m)           examples/utils.py:116-121  (`_B`, frozen)
 *     W_i      (L, h_i, h_{i-1})examples/models/mlp.py:187  (`ws[i]`)
 *     b_i      (L, h_i, 1)      examples/models/mlp.py:189  (`bs[i]`)
 *     scales   (L,)             examples/operator/pde/boundary.py:43 (ExponentialMask), may be NULL
 *     f, Tf    (B, L)           what operator(model, x, importance) returns
 *     lam      (2, L, L)        lam_f1, lam_f2 of methods/nestedlora.py:89
 */
#ifndef NSVD_H
#define NSVD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSVD_ABI_VERSION 6
#define NSVD_MAX_LAYERS 8

#define NSVD_EINVAL (-10001)
#define NSVD_EUNSUPPORTED (-10002)

/* potentials: examples/operator/pde/schrodinger/potentials.py:5-8 and :24-27 */
#define NSVD_POT_HYDROGEN 0 /* V = -Z / |x|  */
#define NSVD_POT_HARMONIC 1 /* V = k |x|^2   */
#define NSVD_POT_ZERO 2     /* V = 0: the infinite well (potentials.py:20-21); the walls are the model's box mask */
#define NSVD_POT_COSINE 3   /* V = sum_d pot_coef[d] cos x_d (potentials.py:30-31)                                     */
#define NSVD_POT_H2_ION 4   /* V = -q / |x - R e_last| - q / |x + R e_last|, q = charge_or_k, R = pot_coef[0]
                             * (potentials.py:11-17)                                                                  */
#define NSVD_POT_SIN_OF_COS 5 /* V = sin(sum_d pot_coef[d] cos x_d) (others.py:33-34): the drift potential of
                               * NSVD_OP_FOKKER_PLANCK, valid with that operator kind only                             */
/* (6 is unassigned) */
#define NSVD_POT_MOLECULE 7 /* V = pot_const - sum_i sum_a Z_a / |r_i - R_a| + sum_{i<j} 1 / |r_i - r_j| over the
                             * n_particles electrons r_i (d = D / n_particles coordinates each) and the n_nuclei rows
                             * (R_a, Z_a) of pot_table (potentials.py:35-57); Schroedinger kind only                    */

/* nsvd_problem.operator_kind */
#define NSVD_OP_SCHROEDINGER 0  /* Tf = -(-scale_kinetic Lap f + V f)            (schrodinger/__init__.py:16-22)      */
#define NSVD_OP_FOKKER_PLANCK 1 /* Tf = fp_scale (Lap f + grad V . grad f + f Lap V), every derivative - those of V
                                 * too - the central difference with step eps (others.py:6-30). Needs eps > 0, no
                                 * Gaussian importance, no box mask and sqrt p >= 1e-5 ("unsupported" otherwise)      */

/* Dirichlet box mask of the model (examples/operator/pde/boundary.py:16-36, --apply_boundary / --boundary_mode):
 * M(x) = prod_d m(clamp(x_d, -lim, lim)), 0 at and beyond the wall, multiplies the model output at every point */
#define NSVD_BOX_NONE 0
#define NSVD_BOX_SQRT 1 /* dir_box_sqrt: m(t) = max((sqrt(2 lim^2 - t^2) - lim) / lim, 0)        */
#define NSVD_BOX_EXP 2  /* dir_box_exp:  m(t) = (1 - exp(-(lim - t))) (1 - exp(-(lim + t)))       */

/* nsvd_problem.use_importance: the density the batch is drawn from and re-weighted by (main_pde.py:89-118) */
#define NSVD_IMP_NONE 0
#define NSVD_IMP_GAUSSIAN 1 /* N(0, sigma^2 I)                                                               */
#define NSVD_IMP_UNIFORM 2  /* uniform on [-sigma, sigma]^D: p = (2 sigma)^-D (sigma = --sampling_scale)      */

/* nesting masks: methods/nestedlora.py:40-54 */
#define NSVD_MASK_CUSTOM 0     /* v (L) and M (L,L) given by pointer                    */
#define NSVD_MASK_SEQUENTIAL 1 /* v = 1, M = triu(1): generated in registers, v/M NULL  */
#define NSVD_MASK_JOINT 2      /* step 1: v_l = (L-l)/L, M = min(v_i, v_j); v/M NULL    */

/* which implementation nsvd_operator_* picks */
#define NSVD_PATH_AUTO 0    /* fused MFMA kernels when the shape allows, else generic   */
#define NSVD_PATH_GENERIC 1 /* layer-by-layer generic kernels (any shape)               */
#define NSVD_PATH_FUSED 2   /* fused MFMA kernels or NSVD_EUNSUPPORTED                  */
#define NSVD_PATH_FUSED_BF16X3 3 /* opt-in, never picked by AUTO: the fused forward with every layer on the bf16 MFMA,
                                  * every float32 operand split into three bf16 planes and six partial products
                                  * accumulated in float32 (f and Tf as close to float64 as the fp32 MFMA's). The
                                  * backward is NSVD_PATH_FUSED's; a fused training step on this path also leaves
                                  * the planes of the updated weights for the next forward (nsvd_step_emits_planes) */
#define NSVD_PATH_GENERIC_EXACT 4 /* opt-in, never picked by AUTO: the exact Laplacian (prob->eps <= 0) on the generic
                                   * kernels - any model validate() accepts, 1 <= D <= 12, every potential, mask and
                                   * importance of the Schroedinger kind. The layers carry D + 2 forward-mode jet streams
                                   * per sample (value, D first derivatives, Laplacian) where the stencil carries 2 D + 1.
                                   * eps > 0 on this path is NSVD_EUNSUPPORTED, as is the Fokker-Planck kind, NeuralEF's
                                   * forward and head-parallel sharding (l_offset / L_total) */

/* Shape of WaveFunctions(ParallelMLP(GaussianFourierFeatureTransform)):
 * examples/operator/pde/__init__.py:19-55, examples/models/mlp.py:167-221, examples/utils.py:90-143 */
typedef struct nsvd_model_desc {
    int32_t L;                       /* --neigs                                        */
    int32_t D;                       /* --ndim * n_particles                           */
    int32_t m;                       /* --fourier_mapping_size                         */
    int32_t nlayers;                 /* number of weight matrices = len(hidden) + 1    */
    int32_t dims[NSVD_MAX_LAYERS];   /* h_0 .. h_{nlayers-1}; the last one must be 1   */
    int32_t has_exp_mask;            /* --apply_exp_mask                               */
    /* ABI 3 (appended; zero = no box mask): the mask belongs to the model, like has_exp_mask - nsvd_model_forward /
     * _backward never see the problem. Alone or inside the exponential mask (boundary.py:51-52). */
    int32_t box_mask;                /* NSVD_BOX_*: --apply_boundary / --boundary_mode */
    float box_lim;                   /* --lim: half-width of the box                   */
} nsvd_model_desc;

/* Device pointers of one parameter set (weights, their gradients, RMSprop state or EMA shadow
 * all use this same struct). */
typedef struct nsvd_params {
    float* fourier_B;                /* (D, m); unused in gradient/state sets          */
    float* W[NSVD_MAX_LAYERS];
    float* b[NSVD_MAX_LAYERS];
    float* scales;                   /* NULL when has_exp_mask == 0                    */
} nsvd_params;

/* OperatorWrapper(NegativeHamiltonian(potential), scale, shift) with Gaussian importance:
 * examples/__init__.py:1-9, examples/operator/pde/schrodinger/__init__.py:4-22,
 * examples/operator/pde/diff_ops.py:4-52, examples/operator/pde/main_pde.py:94-100 */
typedef struct nsvd_problem {
    int32_t potential;               /* NSVD_POT_*                                     */
    float charge_or_k;               /* Z (hydrogen) or k (oscillator)                 */
    float scale_kinetic;             /* problems.py:26 (1.0)                           */
    float eps;                       /* --laplacian_eps: > 0 central differences; <= 0 the exact Laplacian
                                      * (diff_ops.py:7,54-61) by forward-mode jets: the MFMA path (D <= 3), or
                                      * NSVD_PATH_GENERIC_EXACT on explicit request (any model, D <= 12) */
    float op_scale;                  /* --operator_scale                               */
    float op_shift;                  /* --operator_shift                               */
    float sigma;                     /* --sampling_scale of the Gaussian sampler       */
    float hard_mul_const;            /* --hard_mul_const                               */
    int32_t use_importance;          /* NSVD_IMP_*: 0 None, 1 the N(0, sigma^2 I) pdf, 2 the uniform density
                                      * (2 sigma)^-D; sqrt p / max(sqrt p, 1e-5) is kept for all of them. The device
                                      * samplers draw from the same density. */
    /* ABI 4 (appended; all zero = the Schroedinger operator with one of the radial potentials, as before) */
    int32_t operator_kind;           /* NSVD_OP_*                                      */
    float fp_scale;                  /* NegativeLinearFokkerPlanck(scale=...)          */
    float pot_coef[4];               /* cs[d] (cosine, sin-of-cos: float32 values, as torch.tensor(cs) makes them), or R
                                      * in [0] (H2+); entries past D are ignored       */
    /* ABI 5 (appended; all zero = the problems of ABI 4): input dimensions 5 .. 12 in the finite-difference mode and the
     * many-electron potential. Tables longer than pot_coef travel by pointer: the kernels read them with a uniform
     * index from global memory, nothing by-value grows and nothing is copied into a per-thread array. */
    int32_t n_particles;             /* electrons sharing the D coordinates (0 is read as 1): d = D / n_particles is the
                                      * space dimension, and the exponent of the uniform density (2 sigma)^-d
                                      * (main_pde.py:118); the Gaussian density is over all D coordinates */
    int32_t n_nuclei;                /* NSVD_POT_MOLECULE: rows of pot_table           */
    int32_t pot_table_len;           /* floats in pot_table                            */
    float pot_const;                 /* NSVD_POT_MOLECULE: the nuclear repulsion energy (nuclear_energy, host-evaluated) */
    const float* pot_table;          /* DEVICE pointer owned by the caller, stable across graph replays.
                                      * NSVD_POT_COSINE / NSVD_POT_SIN_OF_COS with D > 4: cs[0..D) (float32 values, as
                                      * torch.tensor(cs) makes them; pot_coef is then ignored). NSVD_POT_MOLECULE:
                                      * n_nuclei rows (R_0, .., R_{d-1}, Z). NULL otherwise. */
} nsvd_problem;

int nsvd_abi_version(void);

/* Name of the implementation nsvd_operator_forward would take ("fused_mfma", "generic"). host */
const char* nsvd_path_name(const nsvd_model_desc* desc, int B, int path);
/* The same for a given problem. Input dimensions 5 .. 12 exist in the finite-difference mode (eps > 0): on the generic
 * kernels (NSVD_PATH_AUTO too), and for models the MFMA kernels take on NSVD_PATH_FUSED (the forward in split form, one
 * direction per workgroup); "unsupported" there with eps <= 0, NSVD_PATH_FUSED_BF16X3, NSVD_PATH_FUSED on any other
 * shape, and beyond D = 12; "invalid" for a D > 4
 * cosine / sin-of-cos problem whose pot_table is NULL or not D long, and for a NSVD_POT_MOLECULE problem with
 * n_nuclei < 1, D not a multiple of n_particles, d = D / n_particles not 2 or 3, pot_table_len != n_nuclei (d + 1), a
 * NULL table, or inside the Fokker-Planck kind.
 * The exact-Laplacian mode (prob->eps <= 0) exists on the MFMA path (D <= 3, as the
 * stencil mode: its 3-D form runs one direction per workgroup) and, on explicit request, on the generic kernels:
 * NSVD_PATH_GENERIC_EXACT answers "generic_exact" for eps <= 0 with the Schroedinger kind at any 1 <= D <= 12 and
 * "unsupported" for eps > 0. Every other path value answers as before: "unsupported" when the mode has no path there
 * (NSVD_PATH_AUTO never picks the generic jets); "invalid" for a
 * potential, importance, operator kind or box mask value this library does not know (and for NSVD_POT_SIN_OF_COS
 * outside the Fokker-Planck kind). Every path implements every box mask, potential and importance; entry points that do
 * not (NeuralEF) return NSVD_EUNSUPPORTED. The Fokker-Planck kind is "unsupported" with eps <= 0, Gaussian importance,
 * a box mask, sqrt p < 1e-5 or another potential than NSVD_POT_SIN_OF_COS; the entry points return NSVD_EUNSUPPORTED. */
const char* nsvd_path_name_for(const nsvd_model_desc* desc, const nsvd_problem* prob, int B, int path);

/* Bytes of scratch nsvd_operator_forward / _backward need for batches of up to B rows. */
size_t nsvd_workspace_bytes(const nsvd_model_desc* desc, int B);

/* phiT[(j | m + j), r] = (sin | cos)(x_r . B_j) for the R = E*B stencil rows of x.
 * Replaces GaussianFourierFeatureTransform.forward at the 1+2D points of
 * VectorizedLaplacian.approx_laplacian (examples/utils.py:126-143, diff_ops.py:36-45).
 * phiT: (2m, ldr) feature-major, sample-contiguous; ldr >= E*B. nstencil = 1 (centre only) or E. */
int nsvd_fourier_features(const float* x, const float* fourier_B, float* phiT, int B, int D, int m,
                          float eps, int nstencil, int ldr, void* stream);

/* NEW SYMBOLS ONLY (ABI stays 6). The two kernels of NSVD_PATH_GENERIC_EXACT that are its own (the layers are the generic
 * GEMM's), callable alone. Jet layout: D + 2 column blocks of B samples - block 0 the value, block 1 + d the derivative
 * along x_d, block D + 1 the Laplacian (VectorizedLaplacian.exact_laplacian, diff_ops.py:54-61, in forward mode).
 * nsvd_fourier_features_jets: phiT (2m, ldr) feature-major, ldr >= (D + 2) B: for phi = [sin | cos](x . B_j) the
 * derivative along d is [cos | -sin](x . B_j) B_dj and the Laplacian -|B_j|^2 [sin | cos](x . B_j). Any D >= 1.
 * nsvd_softplus_jets_inplace: z (rows, (D + 2) B), the jet of a hidden layer's pre-activations, becomes the jet of its
 * activations: with s = sigmoid(z0), a = softplus(z0), t_d <- s t_d, l <- s l + s (1 - s) sum_d t_d^2 (the sum over the
 * incoming t_d; torch's softplus threshold 20: s = 1, s (1 - s) = 0 above it). */
int nsvd_fourier_features_jets(const float* x, const float* fourier_B, float* phiT, int B, int D, int m, int ldr,
                               void* stream);
int nsvd_softplus_jets_inplace(float* z, long long rows, int B, int D, void* stream);

/* bit for nsvd_operator_forward's save_for_backward argument: the Fourier features of x are already in
 * the workspace (put there by nsvd_operator_features, typically on another stream while the previous
 * step's optimiser runs - they do not depend on the trainable weights) */
#define NSVD_FEATURES_READY 0x100
/* bit for nsvd_operator_forward's save_for_backward argument, path NSVD_PATH_FUSED_BF16X3 only: the bfloat16 planes of
 * the CURRENT weights are already in this workspace - left there by the nsvd_operator_backward_evd_step[_next] call
 * (same path) that produced these weights, when nsvd_step_emits_planes says it does: the forward then needs no split
 * launch (9 us of 167 at the headline configuration). The caller answers for "current": any other change of the
 * parameters between that step and this forward (a load, another optimiser) invalidates the planes. */
#define NSVD_W_PLANES_READY 0x200
/* Does a fused training step on this shape and path write the planes of the updated weights (1) or not (0)?
 * (NSVD_PATH_FUSED_BF16X3 on a shape the MFMA kernels take, weight gradients without batch slices.) They go into the
 * workspace the next forward reads: `next_ws` of nsvd_operator_backward_evd_step_next, `ws` of .._step. */
int nsvd_step_emits_planes(const nsvd_model_desc* desc, int B, int path);

/* The weight-independent prologue of nsvd_operator_forward alone: Fourier features of the stencil rows of
 * x into `ws`, in the layout the path selected by (desc, B, path) reads. */
int nsvd_operator_features(const nsvd_model_desc* desc, const nsvd_params* params, const nsvd_problem* prob,
                           const float* x, int B, void* ws, size_t ws_bytes, int save_for_backward, int path,
                           void* stream);

/* Tf, f = operator(method, x, importance):  the 1+2D ParallelMLP evaluations, importance
 * re-weighting, central-difference Laplacian, potential, scale/shift
 * (examples/__init__.py:7-9 -> schrodinger/__init__.py:16-22 -> diff_ops.py:9-52 ->
 *  pde/__init__.py:15-16 -> models/mlp.py:204-221).
 * The stencil is the reference's - the same 1 + 2 D points, the same eps - but every path carries the shifted
 * evaluations as EVEN / ODD perturbations of the centre one (z(x +- eps e_d) = z + zE_d +- zO_d through the Fourier map,
 * every layer and the re-weighting), so the float32 result is the stencil's value to ~1e-6 instead of
 * the few per cent a point-wise float32 difference at eps = 0.01 carries (the reference's own float32 Tf is 4e-2 from
 * its float64 Tf: BASELINE.md). f is unaffected. Any eps > 0 (perturbations beyond 0.25 fall back to plain differences).
 * save_for_backward != 0 keeps the centre-row pre-activations in `ws` for nsvd_operator_backward. */
int nsvd_operator_forward(const nsvd_model_desc* desc, const nsvd_params* params,
                          const nsvd_problem* prob, const float* x, int B, float* f, float* Tf,
                          void* ws, size_t ws_bytes, int save_for_backward, int path, void* stream);

/* Parameter gradients of sum(df * f) (f is the only differentiable output: Tf receives no
 * gradient, methods/nestedlora.py:108-111).  Replaces autograd through the centre evaluation.
 * `ws` must be the workspace the matching nsvd_operator_forward(save_for_backward=1) filled.
 * Gradients are OVERWRITTEN (the reference calls optimizer.zero_grad() every step). */
int nsvd_operator_backward(const nsvd_model_desc* desc, const nsvd_params* params,
                           const nsvd_problem* prob, const float* x, int B, const float* df,
                           const nsvd_params* grads, void* ws, size_t ws_bytes, int path, void* stream);

/* out[b, l] = hard_mul_const * base_l(x_b) * mask_l(x_b): WaveFunctions.forward, i.e. what
 * NestedLoRA.forward / method(x) returns (examples/operator/pde/__init__.py:15-16,
 * methods/nestedlora.py:195-200); out: (B, L). save_for_backward != 0 keeps what nsvd_model_backward needs
 * in `ws` (used by compute_loss_kernel-style callers that differentiate through model(x) itself). */
int nsvd_model_forward(const nsvd_model_desc* desc, const nsvd_params* params, const float* x, int B,
                       float hard_mul_const, float* out, void* ws, size_t ws_bytes, int save_for_backward,
                       void* stream);

/* Draws the batch AND prepares its features in one launch: x[b][d] = sigma * N(0,1) with sigma = prob->sigma
 * (prob->use_importance == NSVD_IMP_UNIFORM: sigma * (2 u - 1), u = (23 bits + 1/2) / 2^23 of the same Philox block,
 * never exactly +-sigma: main_pde.py:113-115),
 * from a counter-based generator (Philox4x32-10 + Box-Muller) keyed by (seed, offset, b): the device-side form of
 * `x = sampling_scale * torch.randn(batch_size, ndim)` + host->device copy (examples/operator/pde/main_pde.py:92-93,
 * examples/operator/__init__.py:58). x (B, D) is an OUTPUT; follow with nsvd_operator_forward(... |
 * NSVD_FEATURES_READY). The stream of values is a pure function of (seed, offset): pass a fresh offset per batch;
 * ranks that pass the same (seed, offset) draw the same batch. Not torch's generator: same distribution, different
 * numbers. */
int nsvd_operator_sample_features(const nsvd_model_desc* desc, const nsvd_params* params, const nsvd_problem* prob,
                                  unsigned long long seed, unsigned long long offset, float* x, int B, void* ws,
                                  size_t ws_bytes, int save_for_backward, int path, void* stream);

/* Workspace of nsvd_model_forward / nsvd_model_backward alone (no stencil rows): smaller than
 * nsvd_workspace_bytes, and defined for input dimensions up to 64 (the operator entry points stop at D = 12). */
size_t nsvd_model_workspace_bytes(const nsvd_model_desc* desc, int B);

/* Parameter gradients of sum(dout * model(x)) for the matching nsvd_model_forward(save_for_backward=1). */
int nsvd_model_backward(const nsvd_model_desc* desc, const nsvd_params* params, const float* x, int B,
                        const float* dout, const nsvd_params* grads, void* ws, size_t ws_bytes, void* stream);

/* NestedLoRALossFunctionEVD.forward with f1, f2 = chunk(f, 2) (methods/nestedlora.py:70-94, :263).
 * Stage 1: moments[0 : L*L] = lam_f1, [L*L : 2*L*L] = lam_f2, [2*L*L] = mean_b sum_l v_l f Tf.
 * These 2L^2+1 floats are the data-parallel exchange payload (all-reduce mean over ranks).
 * scratch: nsvd_evd_scratch_bytes(B, L) bytes. */
size_t nsvd_evd_scratch_bytes(int B, int L);
int nsvd_evd_moments(const float* f, const float* Tf, int B, int L, int mask_kind, const float* v,
                     float* moments, void* scratch, void* stream);

/* Stage 2: loss[0] = -2 * moments[2L^2] + sum(M * lam_f1 * lam_f2); loss[1] = operator term,
 * loss[2] = metric term; and, when df != NULL, NestedLoRALossFunctionEVD.backward
 * (methods/nestedlora.py:98-111) with the f1/f2 contributions summed into d loss / d f:
 *   df[b, :] = grad_scale * ( -(4/B) v * Tf[b] + (2/B_half) f[b] @ (M * lam_other) ).
 * grad_scale folds grad_output and, for data parallel runs, nothing else (ranks average later). */
int nsvd_evd_loss_grad(const float* f, const float* Tf, int B, int L, int mask_kind, const float* v,
                       const float* M, const float* moments, float grad_scale, float* loss, float* df,
                       void* stream);

/* Stages 1 + 2 in one call for the single-GPU case (no exchange between them): one launch when
 * B*L <= 16384, the two-stage pipeline otherwise. Same outputs as the two calls above. */
int nsvd_evd_loss_fused(const float* f, const float* Tf, int B, int L, int mask_kind, const float* v,
                        const float* M, float grad_scale, float* moments, float* loss, float* df,
                        void* scratch, void* stream);

/* Stage 1a alone: the per-chunk partial sums of the moments into `scratch` (nsvd_evd_scratch_bytes),
 * without the reduction launch. Consumed by nsvd_operator_backward_evd(moments_reduced = 0). */
int nsvd_evd_partial(const float* f, const float* Tf, int B, int L, int mask_kind, const float* v, void* scratch,
                     void* stream);

/* Heads sharded over `world` processes: gathered = the ranks' packed blocks as an all-gather leaves them,
 * (world, 2, B, L_local) = [rank][f | Tf][row][local head]; writes the (B, world * L_local) arrays f and Tf every
 * other entry point reads and - scratch != NULL - the per-chunk partial moments exactly as nsvd_evd_partial(f, Tf)
 * would (same bits), in the same launch. (The reference has no sharded form: methods/nestedlora.py:70-94 sees the
 * whole (B, L) f.) */
int nsvd_evd_gather_heads(const float* gathered, int world, int B, int L_local, int mask_kind, const float* v,
                          float* f, float* Tf, void* scratch, void* stream);

/* The same for ANY head count L >= world (the reference scripts run --neigs 36 / 55, scripts/exps/pde/hydrogen.sh:28,
 * oscillator.sh:27): rank w owns n_w = L / world + (w < L % world) consecutive heads starting at
 * w (L / world) + min(w, L % world) - the first L % world ranks one head more. `gathered` holds `world` blocks of
 * 2 B ceil(L / world) floats (all-gather blocks are equally long); block w begins with f (B, n_w) then Tf (B, n_w),
 * packed, the rest of a short block is never read. With L % world == 0 this IS nsvd_evd_gather_heads. */
int nsvd_evd_gather_head_blocks(const float* gathered, int world, int B, int L, int mask_kind, const float* v,
                                float* f, float* Tf, void* scratch, void* stream);

/* nsvd_evd_loss_grad + nsvd_operator_backward in ONE call: d loss / d f (methods/nestedlora.py:98-111) is
 * evaluated per sample inside the backward kernels and never stored. `moments` (2L^2+1 floats) is
 *   - an INPUT when moments_reduced != 0 (e.g. after the data-parallel all-reduce of nsvd_evd_moments), or
 *   - an OUTPUT when moments_reduced == 0: the partial sums in `evd_scratch` (from nsvd_evd_partial on the
 *     same f, Tf) are reduced on the fly and the reduced vector is stored here.
 *   - ignored (may be NULL) when moments_reduced == 0 and evd_scratch == NULL ("direct" form, MFMA path only):
 *     every workgroup of the backward takes the 2 L moments of its own head from f itself, no moment kernel
 *     runs at all and `moments` is not written. `loss` (when not NULL, all heads local, one head window) IS: the
 *     workgroups leave per-head partial sums of the two loss terms and the weight-gradient kernel adds them in head
 *     order - the loss value of every step (the reference's loss.item(), examples/operator/__init__.py:74) at no launch.
 * loss[0..2] = {loss, operator term, metric term}. Gradients are overwritten as in nsvd_operator_backward.
 * Head-parallel sharding: f, Tf, v, M and the moments may cover L_total >= desc->L heads, of which this
 * model owns [l_offset, l_offset + desc->L) (f, Tf are then (B, L_total), gathered from all ranks); pass
 * L_total = 0 / l_offset = 0 otherwise. */
int nsvd_operator_backward_evd(const nsvd_model_desc* desc, const nsvd_params* params,
                               const nsvd_problem* prob, const float* x, int B, const float* f, const float* Tf,
                               int mask_kind, const float* v, const float* M, float* moments, int moments_reduced,
                               const void* evd_scratch, int L_total, int l_offset, float grad_scale, float* loss,
                               const nsvd_params* grads, void* ws, size_t ws_bytes, int path, void* stream);

/* nsvd_operator_backward_evd for a WINDOW of heads: only the gradients of heads [l_begin, l_begin + l_count) of
 * this model are produced (all other gradient elements are left untouched). The L heads of ParallelMLP share nothing
 * but the input (examples/models/mlp.py:187-189, 204-221), so autograd's backward of the step
 * (examples/operator/__init__.py:68) splits exactly by head; a sample-sharded run calls this once per window and
 * starts the all-reduce of a window's gradients while the next window is being computed. Calling it for every window
 * of a partition of [0, L) gives bit for bit the gradients of one nsvd_operator_backward_evd call of the same tile
 * shape. Every call must be handed the moments (moments_reduced != 0, or the same evd_scratch): the windows of one
 * step share f, Tf and the workspace of the forward call.
 * nsvd_backward_head_window_ok: 1 when windows of l_count heads are supported for this shape (MFMA path, no split-K
 * partial buffers at that head count), else 0 - the caller then uses one window of all L heads. */
int nsvd_operator_backward_evd_heads(const nsvd_model_desc* desc, const nsvd_params* params,
                                     const nsvd_problem* prob, const float* x, int B, const float* f,
                                     const float* Tf, int mask_kind, const float* v, const float* M, float* moments,
                                     int moments_reduced, const void* evd_scratch, int L_total, int l_offset,
                                     float grad_scale, float* loss, const nsvd_params* grads, void* ws,
                                     size_t ws_bytes, int path, int l_begin, int l_count, void* stream);
int nsvd_backward_head_window_ok(const nsvd_model_desc* desc, const nsvd_problem* prob, int B, int path,
                                 int l_count);

/* nsvd_operator_backward_evd with the optimiser step of nsvd_rmsprop_ema_step taken inside the
 * weight-gradient kernel: each gradient element updates its parameter (params->W/b/scales, IN PLACE), RMSprop
 * square average (opt->sq) and EMA shadow (opt->ema, when has_ema) as it leaves the accumulator, so gradients
 * never make the HBM round trip and the optimiser launch disappears (optimizer.step() + ema.update() of
 * examples/operator/__init__.py:69-73 folded into loss.backward() of :68). Bit-identical to the two separate
 * calls. grads may be NULL on the fused path (gradients are then not stored at all); on the generic path grads
 * is required and the step is taken by per-tensor optimiser launches. lr / ema_decay are the already scheduled
 * values, as for nsvd_rmsprop_ema_step. Not for data-parallel runs (gradients must be all-reduced first). */
typedef struct nsvd_step_state nsvd_step_state;  /* device-resident schedule state, declared below */
typedef struct nsvd_rmsprop {
    nsvd_params sq;                  /* RMSprop square averages, parameter layouts      */
    nsvd_params ema;                 /* EMA shadow parameters (ignored unless has_ema)  */
    double lr, alpha, eps, ema_decay;
    int32_t has_ema;
    /* NULL: lr / ema_decay above are the already scheduled values of this step (kernel arguments).
     * Non-NULL (DEVICE pointer, nsvd_step_state_init): lr, alpha, eps, ema_decay above are ignored; the first
     * backward kernel of the step derives the step's values from state->step, the optimiser epilogue reads them from
     * the device, and the last kernel of the step increments state->step - the call can be captured in a HIP graph
     * and replayed along the schedule. Fused MFMA path only (NSVD_EUNSUPPORTED otherwise). */
    nsvd_step_state* state;
} nsvd_rmsprop;
int nsvd_operator_backward_evd_step(const nsvd_model_desc* desc, const nsvd_params* params,
                                    const nsvd_problem* prob, const float* x, int B, const float* f,
                                    const float* Tf, int mask_kind, const float* v, const float* M,
                                    float* moments, int moments_reduced, const void* evd_scratch, int L_total,
                                    int l_offset, float grad_scale, float* loss, const nsvd_params* grads,
                                    const nsvd_rmsprop* opt, void* ws, size_t ws_bytes, int path, void* stream);

/* ---- device-resident schedule state --------------------------------------------------------------------------
 * What changes from one iteration of the loop body examples/operator/__init__.py:55-74 to the next besides the
 * tensors: CosineAnnealingLR's learning rate (:35,71-72; closed form eta_min + (lr0 - eta_min)(1 + cos(pi t / T)) / 2
 * after t scheduler steps), torch_ema's warmed-up decay min(decay, (1 + n) / (10 + n)) at its n-th update (:36,73),
 * and - for the device sampler - the batch counter. A training step whose kernels take these as launch arguments
 * cannot be replayed from a captured HIP graph. This struct lives in DEVICE memory (the caller allocates
 * sizeof(nsvd_step_state) bytes, 8-byte aligned, and fills it with nsvd_step_state_init); kernels read the step's
 * values from `cur` and the last kernel of a step increments `step`.
 * Arithmetic: the same double-precision expressions the host path evaluates (Python floats), rounded to float32
 * where torch rounds; the device cosine may differ from libm's in the last bit of the DOUBLE, i.e. the float32
 * learning rate agrees with the host path's except with probability ~2^-29 per step. */
struct nsvd_step_state {
    uint64_t step;                   /* optimiser steps taken = scheduler steps = torch_ema.num_updates          */
    uint64_t T_max;                  /* CosineAnnealingLR T_max (--num_iters); 0: constant learning rate          */
    double lr0, eta_min;             /* base learning rate (--lr), CosineAnnealingLR eta_min (0 in the scripts)    */
    double alpha, eps;               /* RMSprop alpha (--rmsprop_decay), eps (1e-10: examples/utils.py:52)         */
    double ema_decay;                /* --ema_decay; the warm-up of torch_ema (use_num_updates=True) is applied    */
    /* the values of the step being taken, derived from `step` by the step's first kernel (or nsvd_step_state_begin): */
    struct {
        float lr, alpha, one_minus_alpha, eps, one_minus_decay, grad_scale;
    } cur;
    uint64_t reserved;
};
/* Fill a device-resident state (one tiny launch on `stream`): counters at `step`, `cur` = the values of step `step`. */
int nsvd_step_state_init(nsvd_step_state* state, double lr0, double eta_min, unsigned long long T_max, double alpha,
                         double eps, double ema_decay, unsigned long long step, void* stream);
/* state->cur <- the values of step state->step (one tiny launch). For loop bodies whose first kernel does not do it:
 * i.e. everything except nsvd_operator_backward_evd_step[_next] with opt->state set. */
int nsvd_step_state_begin(nsvd_step_state* state, void* stream);
/* nsvd_rmsprop_ema_step with the scheduled values read from state->cur (optimizer.step() + scheduler.step() +
 * ema.update() of examples/operator/__init__.py:69-73 in capturable form); advance != 0: this is the last optimiser
 * launch of the step - one thread increments state->step when the kernel is done with it. */
int nsvd_rmsprop_ema_step_dev(float* p, const float* grad, float* sq, float* ema, size_t n, nsvd_step_state* state,
                              double grad_scale, int advance, void* stream);
/* nsvd_operator_sample_features whose batch counter is offset_base + state->step, read on the device: the draw of a
 * captured step moves along with the schedule. */
int nsvd_operator_sample_features_dev(const nsvd_model_desc* desc, const nsvd_params* params,
                                      const nsvd_problem* prob, unsigned long long seed,
                                      unsigned long long offset_base, const nsvd_step_state* state, float* x, int B,
                                      void* ws, size_t ws_bytes, int save_for_backward, int path, void* stream);

/* torch.optim.RMSprop(alpha, eps, momentum=0, centered=False) step + torch_ema update, fused
 * (examples/utils.py:50-57, examples/operator/__init__.py:69-73):
 *   g = grad_scale * grad; sq = alpha sq + (1-alpha) g^2; p -= lr g / (sqrt(sq) + eps);
 *   ema -= (1 - ema_decay) (ema - p)        (skipped when ema == NULL)
 * over n contiguous floats. lr is the already-scheduled learning rate, ema_decay the already
 * warmed-up decay min(decay, (1+t)/(10+t)). Host scalars are doubles (Python floats) and are rounded
 * to float32 exactly where torch rounds them: alpha, (1 - alpha), lr, eps, (1 - ema_decay). */
int nsvd_rmsprop_ema_step(float* p, const float* grad, float* sq, float* ema, size_t n, double lr,
                          double alpha, double eps, double ema_decay, double grad_scale, void* stream);

/* ---- the other optimisers of the reference's PDE loop (examples/utils.py:48-72: --optimizer rmsprop | adam | sgd,
 * --momentum), stand-alone over n contiguous floats. torch.optim's rules as get_optimizer configures them (weight_decay
 * 0, dampening 0, no Nesterov, no amsgrad, not centred), followed by the torch_ema update; g = grad_scale * grad:
 *   NSVD_OPT_SGD,     momentum 0: p -= lr g                                                        (no state)
 *   NSVD_OPT_SGD,     momentum u: mom = g on the first step taken, else u mom + g; p -= lr mom      (mom)
 *   NSVD_OPT_RMSPROP, momentum 0: nsvd_rmsprop_ema_step                                            (sq)
 *   NSVD_OPT_RMSPROP, momentum u: sq = alpha sq + (1-alpha) g^2; mom = u mom + g / (sqrt(sq) + eps); p -= lr mom
 *                                                                                                   (sq, mom)
 *   NSVD_OPT_ADAM: mom += (1-beta1)(g - mom); sq = beta2 sq + (1-beta2) g^2; t = steps taken + 1;
 *                  p -= (lr / (1 - beta1^t)) mom / (sqrt(sq) / sqrt(1 - beta2^t) + eps)             (sq = v, mom = m)
 * State slots a rule does not use may be NULL and are never touched. Host scalars are doubles (Python floats); lr /
 * (1 - beta1^t) and sqrt(1 - beta2^t) are formed in double precision, and everything is rounded to float32 where torch
 * rounds: lr, alpha, 1 - alpha, eps, momentum, 1 - beta1, beta2, 1 - beta2, the two Adam scalars, 1 - ema_decay. */
#define NSVD_OPT_RMSPROP 0
#define NSVD_OPT_SGD 1
#define NSVD_OPT_ADAM 2
typedef struct nsvd_opt_config {
    int32_t kind;          /* NSVD_OPT_*; anything else: NSVD_EINVAL                                              */
    int32_t reserved0;
    double lr;             /* nsvd_opt_step: the step's already scheduled learning rate; _state_init: the base one */
    double alpha;          /* RMSprop alpha (--rmsprop_decay)                                                      */
    double eps;            /* RMSprop eps (1e-10: examples/utils.py:52) / Adam eps (--adam_eps)                    */
    double momentum;       /* SGD / RMSprop --momentum                                                             */
    double beta1, beta2;   /* Adam betas (0.9, 0.999)                                                              */
    double ema_decay;      /* nsvd_opt_step: the already warmed-up decay; _state_init: --ema_decay                 */
} nsvd_opt_config;
/* One step of cfg's rule; steps_taken: optimiser steps before this one (SGD's first-step rule, Adam's t - 1). */
int nsvd_opt_step(float* p, const float* grad, float* sq, float* mom, float* ema, size_t n, const nsvd_opt_config* cfg,
                  unsigned long long steps_taken, double grad_scale, void* stream);

/* The device-resident schedule of any rule (what nsvd_step_state is for RMSprop without momentum): beside the cosine
 * learning rate and the EMA warm-up, Adam's bias corrections and SGD's first-step flag move along with `step`. Derived
 * in double precision by one thread, with the expressions nsvd_opt_step evaluates on the host. DEVICE memory,
 * sizeof(nsvd_opt_state) bytes, 8-byte aligned, filled by nsvd_opt_state_init. */
typedef struct nsvd_opt_state {
    uint64_t step;                   /* optimiser steps taken = scheduler steps = torch_ema.num_updates             */
    uint64_t T_max;                  /* CosineAnnealingLR T_max; 0: constant learning rate                           */
    double lr0, eta_min;
    double alpha, eps, ema_decay, momentum, beta1, beta2;
    int32_t kind;                    /* NSVD_OPT_*                                                                   */
    int32_t mismatch;                /* set by a nsvd_opt_step_dev launch whose cfg names another rule (it did nothing) */
    /* the values of the step being taken, derived from `step` by nsvd_opt_state_begin: */
    struct {
        float lr, alpha, one_minus_alpha, eps, one_minus_decay, grad_scale;
        float momentum, one_minus_beta1, beta2, one_minus_beta2, step_size, bc2_sqrt;
        int32_t first_step, rule;
    } cur;
} nsvd_opt_state;
/* Fill a device-resident state (one tiny launch): counters at `step`, `cur` = the values of step `step`. */
int nsvd_opt_state_init(nsvd_opt_state* state, const nsvd_opt_config* cfg, double eta_min, unsigned long long T_max,
                        unsigned long long step, void* stream);
/* state->cur <- the values of step state->step (one tiny launch; first thing in a captured loop body). */
int nsvd_opt_state_begin(nsvd_opt_state* state, void* stream);
/* nsvd_opt_step with the step's scalars read from state->cur (capturable: nothing host-side changes between replays).
 * cfg: the configuration the state was initialised with - it selects the kernel and which slots must be non-NULL; a
 * launch whose rule is not the state's touches nothing but state->mismatch. advance != 0: last optimiser launch of the
 * step - one thread increments state->step when the kernel is done with it. */
int nsvd_opt_step_dev(float* p, const float* grad, float* sq, float* mom, float* ema, size_t n,
                      const nsvd_opt_config* cfg, nsvd_opt_state* state, double grad_scale, int advance, void* stream);

/* nsvd_operator_backward_evd_step for any rule of nsvd_opt_config: the optimiser + EMA update taken inside the
 * backward. On the MFMA kernels every gradient element is applied to its parameter in the weight-gradient kernel's
 * epilogue (with `grads` NULL no gradient reaches memory); on the generic kernels the gradients are stored (`grads`
 * required) and one stand-alone launch per tensor follows. State tensors are in the parameters' layouts; tables of
 * slots the rule does not use are ignored. */
typedef struct nsvd_optimizer {
    nsvd_opt_config cfg;      /* lr: the step's scheduled learning rate, ema_decay: the already warmed-up decay      */
    nsvd_params sq;           /* RMSprop's square averages / Adam's exp_avg_sq                                        */
    nsvd_params mom;          /* momentum buffers / Adam's exp_avg                                                    */
    nsvd_params ema;          /* EMA shadow (has_ema != 0)                                                            */
    int32_t has_ema;
    int32_t reserved0;
    uint64_t steps_taken;     /* optimiser steps before this one (SGD's first-step rule, Adam's t - 1)                */
    /* Non-NULL (DEVICE pointer, nsvd_opt_state_init with this cfg's rule): cfg.lr, cfg.ema_decay and steps_taken are
     * ignored - the step's scalars are derived on the device (one tiny launch before the step's first kernel) and the
     * step's last kernel increments state->step. NSVD_OPT_RMSPROP without momentum has its own device-resident form
     * (nsvd_rmsprop::state of nsvd_operator_backward_evd_step): with a state here it returns NSVD_EUNSUPPORTED. */
    nsvd_opt_state* state;
} nsvd_optimizer;
/* x_next NULL: the counterpart of nsvd_operator_backward_evd_step. x_next non-NULL: the counterpart of
 * nsvd_operator_backward_evd_step_next (the next batch's draw and features ride in the chain launch; MFMA kernels
 * only). NSVD_OPT_RMSPROP without momentum takes the kernels of nsvd_operator_backward_evd_step: same bits. */
int nsvd_operator_backward_evd_opt_step(const nsvd_model_desc* desc, const nsvd_params* params,
                                        const nsvd_problem* prob, const float* x, int B, const float* f,
                                        const float* Tf, int mask_kind, const float* v, const float* M,
                                        float* moments, int moments_reduced, const void* evd_scratch, int L_total,
                                        int l_offset, float grad_scale, float* loss, const nsvd_params* grads,
                                        const nsvd_optimizer* opt, void* ws, size_t ws_bytes, int path,
                                        unsigned long long next_seed, unsigned long long next_offset, float* x_next,
                                        void* ws_next, size_t ws_next_bytes, void* stream);

/* compute_spectrum_evd accumulation for one chunk (methods/spectrum.py:56-75):
 *   w = sqrt(p_train(x)) / sqrt(p_val), phi = nan_to_num(w f), Tphi = nan_to_num(w Tf),
 *   Tphi rows with x ~ 0 zeroed, cov += phi^T phi, quad += phi^T Tphi   (cov, quad: (L, L)).
 * p_val = uniform on [-lim, lim]^D (main_pde.py:129-130).
 * use_importance (all three entry points): NSVD_IMP_NONE (p_train = 1) or NSVD_IMP_GAUSSIAN (the N(0, sigma^2 I) pdf,
 * evaluated in the kernel). NSVD_IMP_UNIFORM returns NSVD_EUNSUPPORTED - that density is a constant: weight the rows
 * by sqrt(p_train) and pass NSVD_IMP_NONE - and any other value NSVD_EINVAL; nothing is launched. L <= 64. */
int nsvd_spectrum_accumulate(const float* f, const float* Tf, const float* x, int B, int L, int D,
                             float sigma, int use_importance, float lim, float* cov, float* quad,
                             void* stream);
/* The same accumulation with float64 products, sums and accumulators (cov, quad: (L, L) doubles). The reference keeps
 * float32 accumulators (methods/spectrum.py:60-61,74-75); for excited states diag(quad) is a sum of terms up to 10^2 x
 * larger than itself, which a float32 running sum carries to ~1e-4 only - the evaluation paths of this package
 * (trainer.spectrum, spectrum.compute_spectrum_evd) accumulate here and round once at the end. */
int nsvd_spectrum_accumulate_f64(const float* f, const float* Tf, const float* x, int B, int L, int D,
                                 float sigma, int use_importance, float lim, double* cov, double* quad,
                                 void* stream);
/* compute_spectrum_evd(set_first_mode_const=True) (methods/spectrum.py:68-70): the same float64 accumulation with a
 * constant-one column padded in FRONT of the weighted phi and Tphi (after the weighting, before nan_to_num and the
 * x ~ 0 zeroing of Tphi); cov, quad: (L + 1, L + 1) doubles. */
int nsvd_spectrum_accumulate_const_f64(const float* f, const float* Tf, const float* x, int B, int L, int D,
                                       float sigma, int use_importance, float lim, double* cov, double* quad,
                                       void* stream);

/* ---- eigenFUNCTION accuracy against the analytic ground truths (2-D problems) ----------------------------------
 * Replaces, on the device and per chunk of the validation grid, the host evaluation of the reference's
 * examples/operator/pde/schrodinger/ground_truths.py - Hydrogen2D.eigfunc (:134-149), HarmonicOscillator._eigfunc_1d /
 * _eigfunc_2d (:96-107), InfiniteWell2D.eigfunc (:61-63) - and the (n, L) products that examples/linalg.py's
 * subspace_distance (:5-8), rotate (:11-16) and procrustes (:19-28) take: three small float64 matrices are left, from
 * which neural_svd_amd/eigfuncs.py computes those metrics. NEW SYMBOLS ONLY: NSVD_ABI_VERSION stays 6.
 *
 * kind / param: NSVD_GT_HYDROGEN2D with the charge Z (psi_Z(x) = Z psi_1(Z x)), NSVD_GT_HARMONIC2D with k of
 * V = k |x|^2 (b = sqrt(k) in the reference's formula), NSVD_GT_WELL2D with the half-width lim of the box [-lim, lim]^2
 * (psi = (1 / lim) sin(nx pi (x + lim) / (2 lim)) sin(ny pi (y + lim) / (2 lim)), 0 outside).
 * qnums: HOST pointer to (Lg, 2) ints - (n, l), (nx, ny), (nx, ny) - 1 <= Lg <= 80 (NSVD_EUNSUPPORTED above). Lg may
 * exceed L: a metric over a degenerate level needs the whole level. Admitted: hydrogen 0 <= n <= 16, |l| <= n (l < 0
 * keeps the reference's sin(l th), negative l inside); oscillator 0 <= nx, ny <= 16; well 1 <= nx, ny <= 32. The
 * library computes each function's float64 normalisation on the host (lgamma) and hands the table to the kernel BY
 * VALUE in the launch arguments: no allocation, no copy, no synchronisation; legal on any stream and under capture.
 * The float32 coordinates are widened to float64 and everything after that is float64: Laguerre and Hermite by their
 * three-term recurrences, cos(l th) and sin(l th) from x / r and y / r by the Chebyshev recurrence. At r = 0 hydrogen
 * returns the limit (the reference's formula gives NaN for l = 0: 0 * log 0): the finite value for l = 0, 0 otherwise.
 * The far tail underflows to 0, never to NaN.
 * NSVD_EINVAL: a null pointer, B, L or Lg <= 0, an unknown kind, param not positive and finite, a quantum number the
 * kind does not admit. A refused call launches nothing and writes nothing. */
#define NSVD_GT_HYDROGEN2D 0
#define NSVD_GT_HARMONIC2D 1
#define NSVD_GT_WELL2D 2
/* psi (B, Lg) float64 row-major: psi[b][i] = function i at x[b] (x: (B, 2) float32). */
int nsvd_eigfunc_eval(int kind, double param, const int* qnums, int Lg, const float* x, int B, double* psi,
                      void* stream);
/* One pass over a chunk. With w and phi = nan_to_num(w f) exactly as nsvd_spectrum_accumulate forms them
 * (w = sqrt(p_train(x)) / sqrt(p_val), D = 2) and psi_w = psi / sqrt(p_val):
 *   gram (Lg, Lg) += psi_w^T psi_w,  cross (Lg, L) += psi_w^T phi,  cov (L, L) += phi^T phi   (cov may be NULL)
 * float64 products, sums and accumulators; the sum across workgroups is a float64 atomic +=, as
 * nsvd_spectrum_accumulate_f64's (the order is not fixed). f: (B, L) float32, L <= 64 (NSVD_EUNSUPPORTED above).
 * use_importance: the three-way rule of nsvd_spectrum_accumulate (NONE and GAUSSIAN in the kernel, UNIFORM
 * NSVD_EUNSUPPORTED, anything else NSVD_EINVAL). */
int nsvd_eigfunc_accumulate_f64(int kind, double param, const int* qnums, int Lg, const float* f, int L,
                                const float* x, int B, float sigma, int use_importance, float lim, double* gram,
                                double* cross, double* cov, void* stream);

/* ---- the same for the 3-D hydrogen atom: three quantum numbers, x (B, 3) ---------------------------------------
 * Replaces the host evaluation of ground_truths.py's Hydrogen3D.eigfunc (:177-193) with its real spherical harmonics
 * (real_sph_harm / sph_harm, :218-270; cartesian_to_spherical :204-209), which the reference defines and never
 * evaluates (its validation grid stops at ndim 2), and the same (n, L) products of examples/linalg.py as above.
 * NEW SYMBOLS ONLY: NSVD_ABI_VERSION stays 6. Entry points of their own, and a kind that is not 3: the two above keep
 * their (Lg, 2) table and keep refusing every kind but their three with NSVD_EINVAL; these two refuse the 2-D kinds.
 *
 * kind: NSVD_GT_HYDROGEN3D; param: the charge Z of -lap - Z / r. qnums: HOST pointer to (Lg, 3) ints (n, l, m),
 * 1 <= n <= 16, 0 <= l < n, |m| <= l, 1 <= Lg <= 80 (NSVD_EUNSUPPORTED above). With rho = Z r / n, a = |m|:
 *   psi = norm rho^l exp(-rho / 2) L_{n-l-1}^(2l+1)(rho) P_l^a(z / r) ang
 *   norm = sqrt((Z/n)^3 / (2n)) sqrt((n-l-1)! / (n+l)!) sqrt((2l+1) / (4 pi) (l-a)! / (l+a)!)
 *   ang = 1 (m = 0), sqrt(2) cos(a phi) (m < 0), -sqrt(2) sin(a phi) (m > 0): the reference's pairing
 * P_l^a without the Condon-Shortley phase, by its recurrence in l from P_a^a = (2a-1)!! sin^a(theta); Laguerre by its
 * recurrence; cos / sin of a phi by the Chebyshev recurrence on x / s, y / s, s = sqrt(x^2 + y^2) (no atan2). Float32
 * coordinates widened to float64, float64 throughout; the normalisations are computed on the host (lgamma) and travel
 * BY VALUE in the launch arguments (80 x 24 bytes): no allocation, no copy, no synchronisation; legal on any stream
 * and under capture. Limits, the reference's own values: at r = 0 the finite value for l = 0 and exactly 0 otherwise;
 * on the z axis phi = 0; past rho = 1500 the value is 0, never NaN.
 * NSVD_EINVAL: a null pointer, B, L or Lg <= 0, any other kind, param not positive and finite, a quantum number
 * outside the ranges above. A refused call launches nothing and writes nothing. */
#define NSVD_GT_HYDROGEN3D 8
/* psi (B, Lg) float64 row-major: psi[b][i] = function i at x[b] (x: (B, 3) float32). */
int nsvd_eigfunc3_eval(int kind, double param, const int* qnums, int Lg, const float* x, int B, double* psi,
                       void* stream);
/* nsvd_eigfunc_accumulate_f64 with x (B, 3): p_val = (2 lim)^-3 and the Gaussian density over three coordinates
 * (w and phi exactly as nsvd_spectrum_accumulate forms them at D = 3). Everything else as there: float64 products and
 * atomics, L <= 64, cov may be NULL, the three-way rule for use_importance. */
int nsvd_eigfunc3_accumulate_f64(int kind, double param, const int* qnums, int Lg, const float* f, int L,
                                 const float* x, int B, float sigma, int use_importance, float lim, double* gram,
                                 double* cross, double* cov, void* stream);

/* ---- next row: dense kernel operator on a minibatch (kernel-operator configuration) ---------------------------
 * Kf[i][l] = scale * sum_k K[rows[i]][cols[k]] f[k][l]: the (Kf, f) producer that
 * NestedLoRA.compute_loss_kernel's `get_approx_kernel_op(x)(model, x, importance)` contract consumes
 * (methods/nestedlora.py:230-252; split_batch: rows = x1, cols = x2, f = model(x2), scale = 1 / B2). The reference
 * ships no kernel operator; the definition is this build's (K = A A^T / r + 1e-3 I on N points,
 * minibatch of indices drawn with replacement), restated in float64 by oracle/nsvd_oracle.py:kernel_apply.
 * K: (N, ldk) row-major float32, ldk >= N rounded up to 64 (rows are read in whole 64-float chunks; the padding
 * may hold anything finite), 16-byte aligned; rows (B1), cols (B2): int64 point indices; f: (B2, L); out: (B1, L).
 * Indices outside [0, N) contribute / produce zeros. */
size_t nsvd_kernel_apply_workspace_bytes(int N, int B1, int L);
int nsvd_kernel_apply(const float* K, size_t ldk, int N, const long long* rows, int B1, const long long* cols,
                      int B2, const float* f, int L, float scale, float* out, void* ws, size_t ws_bytes,
                      void* stream);

/* ---- next row: matrix-free radial kernel operator on coordinate batches (ABI 6) -------------------------------
 * out[i][l] = scale * sum_j k(|x_i - y_j|) f[j][l]: the (Kf, f) producer of the same consumer contract
 * (methods/nestedlora.py:230-252; x = x1, y = x2, f = model(x2), scale = 1 / B2) for a kernel given by a formula on
 * coordinates drawn fresh every step - the definition oracle/nsvd_oracle.py:gaussian_kernel_apply restates in float64.
 * NSVD_RBF_GAUSSIAN: k = exp(-d^2 / (2 ell^2)); NSVD_RBF_EXPONENTIAL: k = exp(-d / ell); d = |x_i - y_j| from direct
 * differences (translation invariant). x: (B1, D), y: (B2, D), f: (B2, L), out: (B1, L), float32 row-major; x == y is
 * allowed, out must not alias an input. Any B1, B2, L >= 1; 1 <= D <= 64 (NSVD_EUNSUPPORTED above); ell > 0. The
 * (B1, B2) kernel matrix is never stored; partial sums over slices of the reference rows are reduced in slice order
 * (no atomics: bit-reproducible). The workspace (256-byte aligned) holds padded copies of y and f^T and the partial
 * tiles; its size is 0 for shapes outside these ranges. */
#define NSVD_RBF_GAUSSIAN 0
#define NSVD_RBF_EXPONENTIAL 1
size_t nsvd_rbf_apply_workspace_bytes(int B1, int B2, int D, int L);
int nsvd_rbf_apply(const float* x, int B1, const float* y, int B2, int D, const float* f, int L, int kind, float ell,
                   float scale, float* out, void* ws, size_t ws_bytes, void* stream);

/* ---- next row: two-sided matrix-free radial kernel operator: both halves of a kernel SVD step ------------------------
 * out_x[i][l] = scale_g * sum_j k(|x_i - y_j|) g[j][l]   (B1, L)   "K g"
 * out_y[j][l] = scale_f * sum_i k(|x_i - y_j|) f[i][l]   (B2, L)   "K^T f"
 * - the (Tg, Tadjf) producer of NestedLoRALossFunctionSVD(f, Tg, g, Tadjf) (methods/nestedlora.py:100-156; f = f(x),
 * g = g(y), scale_g = 1 / B2, scale_f = 1 / B1) for a cross-domain kernel k(x, y) with x and y drawn from different
 * measures; restated in float64 by tests/_pair_oracle.py. Kinds, distances, the exponent constant, ranges, error codes
 * and the workspace rules are nsvd_rbf_apply's: x: (B1, D), y: (B2, D), g: (B2, L), f: (B1, L), float32 row-major; x may
 * be y and f may be g; the outputs must not alias an input or each other. Every kernel value is evaluated once per 64
 * heads and feeds both contractions; what crosses workgroups goes through partial copies in the workspace (at most 32 of
 * either output, whatever the shape) that a second launch adds in a fixed order: no atomics, bit-reproducible. No
 * allocation, no synchronisation; a refused call writes nothing. NEW SYMBOLS ONLY: NSVD_ABI_VERSION stays 6.
 * nsvd_rbf_apply_pair_partition (host only) reports how a call of that shape splits the work: row_groups runs of x tiles
 * (= partial copies of out_y) and col_slices runs of y rows (= partial copies of out_x). */
size_t nsvd_rbf_apply_pair_workspace_bytes(int B1, int B2, int D, int L);
int nsvd_rbf_apply_pair_partition(int B1, int B2, int D, int L, int* row_groups, int* col_slices);
int nsvd_rbf_apply_pair(const float* x, int B1, const float* y, int B2, int D, const float* g, const float* f, int L,
                        int kind, float ell, float scale_g, float scale_f, float* out_x, float* out_y, void* ws,
                        size_t ws_bytes, void* stream);

/* ---- next row: matrix-free dot-product kernel operator on coordinate batches ----------------------------------------
 * out[i][l] = scale * sum_j k(x_i, y_j) f[j][l] for a kernel of the inner product x.y - the other family kernel
 * eigenfunction work is run on (polynomial and neural-network Gaussian-process kernels) - on the same consumer contract
 * and with the conventions of nsvd_rbf_apply: x: (B1, D), y: (B2, D), f: (B2, L), out: (B1, L), float32 row-major;
 * x == y is allowed, out must not alias an input. Any B1, B2, L >= 1; 1 <= D <= 64 (NSVD_EUNSUPPORTED above, workspace
 * size 0). x.y is formed on the fp32 MFMA (an inner product has no cancellation to protect), the map is applied in
 * registers and the (B1, B2) kernel matrix is never stored; partial sums over slices of the reference rows are reduced
 * in slice order (no atomics: bit-reproducible). The workspace is 256-byte aligned. NSVD_EINVAL: a null pointer, a
 * non-positive size, an unknown kind (2 is unassigned), (polynomial kind) a degree outside 1..8 or a non-finite gamma or
 * coef0, (deep ReLU kinds) a depth outside 1..8, a gamma that is not finite and positive or a coef0 that is not finite
 * and non-negative, a short or misaligned workspace. A refused call writes nothing. NEW SYMBOLS ONLY: NSVD_ABI_VERSION stays 6.
 * Numerical rules (restated in float64 by tests/_dot_oracle.py):
 * - NSVD_DOT_POLYNOMIAL: the integer power is taken by multiplication (no pow, exp or log); the result is whatever
 *   float32 gives for finite inputs.
 * - NSVD_DOT_ARCCOS1: cos t is clamped to [-1, 1]; the bracket sin t + (pi - t) cos t (non-negative in exact
 *   arithmetic, ~(pi - t)^3 / 3 near antiparallel rows) is clamped at 0 from below; a row of zero norm on either side
 *   gives exactly 0, never a NaN. The kind is well conditioned at both ends: at t -> 0 the bracket is
 *   pi (1 - t^2 / 2), so the ~4e-4 that float32 leaves in t on the diagonal costs 1e-7.
 * - The ORDER-0 arc-cosine kernel (1 - t / pi) is deliberately NOT offered, and is not a one-line addition: on the
 *   diagonal it turns that 4e-4 in t into a 1e-4 error of the kernel value, and repairing it needs the angle from direct
 *   differences of normalised rows - the radial kernel's VALU cost again.
 * - NSVD_DOT_RELU_NNGP, NSVD_DOT_RELU_NTK: the NNGP kernel S_depth and the neural tangent kernel T_depth of a ReLU
 *   network `depth` layers deep, weight variance gamma > 0, bias variance coef0 >= 0. These kinds read gamma, coef0 and,
 *   IN THE degree SLOT, depth (1..8). With A1(c) = (sin t + (pi - t) cos t) / pi and A0(c) = (pi - t) / pi, cos t = c
 *   clamped to [-1, 1] (Cho & Saul's orders 1 and 0), S_0 = T_0 = x.y, q_0(v) = |v|^2, and for l = 1 .. depth
 *       p = sqrt(q_{l-1}(x) q_{l-1}(y)),  c = S_{l-1} / p,  S_l = gamma p A1(c) + coef0,
 *       T_l = S_l + gamma T_{l-1} A0(c),  q_l(v) = gamma q_{l-1}(v) + coef0  (= S_l(v, v): the diagonal in closed form).
 *   Conventions: S_0 is x.y itself (no input-layer variance), and where p = 0 (a zero row at level 1; with coef0 = 0 at
 *   every level) both A terms are taken as 0: S_l = T_l = coef0, never a NaN. gamma = 1, coef0 = 0, depth = 1 makes the
 *   NNGP kind NSVD_DOT_ARCCOS1 (to rounding: p is one root of the product here). Per level the bracket is clamped at 0
 *   and sin t, pi - t come from the same clamped c, as for NSVD_DOT_ARCCOS1. The NNGP kind is as well conditioned as
 *   that kind. The NTK kind is NOT, by the argument of the paragraph above: A0 = acos(-c) / pi has an unbounded slope
 *   at c = +-1, so an error delta of the float32 c becomes sqrt(2 delta) / pi in A0 - about 2e-4 per level where x_i
 *   meets itself (c = 1 - 1.2e-7), on near-parallel pairs, and on every pair at D = 1. That is a property of forming c
 *   from a float32 x.y, shared by a float32 composition from library calls, and it is left as it is: no special case
 *   for x == y, no distance-based 1 - c. Away from c = +-1 both kinds meet the bound of the other kinds. */
#define NSVD_DOT_POLYNOMIAL 0   /* k = (gamma * x.y + coef0)^degree, integer degree in 1..8 */
#define NSVD_DOT_ARCCOS1    1   /* k = |x||y| / pi * (sin t + (pi - t) cos t), cos t = x.y / (|x||y|): Cho & Saul's
                                   order-1 arc-cosine kernel = 2 E_w[relu(w.x) relu(w.y)], w ~ N(0, I): the NNGP kernel
                                   of one ReLU layer. gamma, coef0, degree ignored. */
/* (2 is unassigned: NSVD_EINVAL) */
#define NSVD_DOT_RELU_NNGP  3   /* k = S_depth: the NNGP kernel of a ReLU network `depth` layers deep (gamma: weight
                                   variance, coef0: bias variance, degree: the depth, 1..8) */
#define NSVD_DOT_RELU_NTK   4   /* k = T_depth: the neural tangent kernel of the same network */
size_t nsvd_dot_apply_workspace_bytes(int B1, int B2, int D, int L);
int nsvd_dot_apply(const float* x, int B1, const float* y, int B2, int D, const float* f, int L, int kind,
                   float gamma, float coef0, int degree, float scale, float* out, void* ws, size_t ws_bytes,
                   void* stream);

/* ---- next row: two-sided matrix-free dot-product kernel operator: both halves of a kernel SVD step -------------------
 * out_x[i][l] = scale_g * sum_j k(x_i, y_j) g[j][l]   (B1, L)   "K g"
 * out_y[j][l] = scale_f * sum_i k(x_i, y_j) f[i][l]   (B2, L)   "K^T f"
 * - nsvd_rbf_apply_pair for the kernels of the inner product. Kinds, numerical rules (the power by multiplication, the
 * clamps, a row of zero norm on either side gives exactly 0), ranges (1 <= D <= 64, any B1, B2, L >= 1) and error codes
 * are nsvd_dot_apply's; operand shapes (x: (B1, D), y: (B2, D), g: (B2, L), f: (B1, L), float32 row-major), aliasing
 * rules (x may be y and f may be g; an output that overlaps an input or the other output is NSVD_EINVAL) and the
 * partition query are nsvd_rbf_apply_pair's. Every x_i . y_j is formed once per 64 heads on the fp32 MFMA, mapped once
 * in registers and feeds both contractions; rows that only pad a tile are forced to 0 on BOTH sides, so a kernel value
 * that overflows (coef0^degree) reaches the rows it belongs to and no other. Partial copies in the workspace (at most 32
 * of either output, whatever the shape) are added in a fixed order by a second launch: no atomics, bit-reproducible.
 * No allocation, no synchronisation; a refused call writes nothing. Restated in float64 by tests/_dot_pair_oracle.py.
 * NEW SYMBOLS ONLY: NSVD_ABI_VERSION stays 6. */
size_t nsvd_dot_apply_pair_workspace_bytes(int B1, int B2, int D, int L);
int nsvd_dot_apply_pair_partition(int B1, int B2, int D, int L, int* row_groups, int* col_slices);
int nsvd_dot_apply_pair(const float* x, int B1, const float* y, int B2, int D, const float* g, const float* f, int L,
                        int kind, float gamma, float coef0, int degree, float scale_g, float scale_f, float* out_x,
                        float* out_y, void* ws, size_t ws_bytes, void* stream);

/* ---- next row: the dense side of the Nystrom baseline (methods/nystrom.py:8-47) -------------------------------------
 * The reference's Nystrom.evd forms the n x n Gram matrix and calls a host eigh on it; here the top L <= 64 eigenpairs of
 * G = k(xs, xs) / n come from block subspace iteration with Rayleigh-Ritz on a basis V (n, m), m <= 80, with
 * W = G V from nsvd_rbf_apply (neural_svd_amd/nystrom.py drives the loop). These are the three pieces beside that
 * product. NEW SYMBOLS ONLY: no existing entry point, struct or constant changes, so NSVD_ABI_VERSION stays 6.
 *
 * nsvd_tsgram_f64: XtX = X^T X and XtY = X^T Y, (m, m) float64 row-major, of X, Y (n, m) float32 with row strides
 *   ldx, ldy >= m (in floats). Either output may be NULL (Y may then be NULL too). Products and sums in float64; the
 *   rows are split over workgroups and the partial matrices reduced in slice order by a second launch (no atomics:
 *   bit-reproducible). 1 <= m <= 80 (NSVD_EUNSUPPORTED above), any n >= 1. Workspace 256-byte aligned; its size is 0
 *   for shapes outside these ranges.
 * nsvd_ritz_step_f64: one workgroup, float64, everything (m, m) contiguous row-major:
 *       eigh((A + A^T) / 2) = Q diag(theta) Q^T, theta descending, ties by ascending index (cyclic Jacobi in a fixed
 *       round-robin ordering, at most 30 sweeps, until |off-diagonal|_F <= 1e-15 |A|_F);
 *       M = Q^T S Q;  resid_k = sqrt(max(M_kk - theta_k^2 (2 - q_k^T C q_k), 0));  R = chol(M) (upper);  T = Q R^-1.
 *   With S = W^T W, A = V^T W and C = V^T V: (theta_k, V q_k) are the Ritz pairs, resid_k = |W q_k - theta_k V q_k|, and
 *   W T is an orthonormal basis of span(W) whose leading columns are the Ritz directions in order. C == NULL stands for
 *   C = I (resid_k = sqrt(max(M_kk - theta_k^2, 0))): exact for an orthonormal V, but a V stored in float32 is
 *   orthonormal to ~1e-8 only, and the square root turns that into a floor of ~1e-4 theta_k under the residuals -
 *   pass the Gram matrix of the stored V to have them to ~1e-8.
 *   A == NULL: orthonormalisation only (Q = I, theta = resid = 0, T = chol(S)^-T). theta, resid, Q may be NULL.
 *   *status (device int, zeroed by the caller) has NSVD_RITZ_* bits OR-ed in, so that one read can cover several
 *   calls. On a non-positive (or non-finite) pivot T is zero from that column on and nothing non-finite is stored in T.
 *   Every loop of the kernel has a trip count bounded by m or a constant.
 * nsvd_ts_rotate: out (n, k) = X (n, m) T[:, :k], T float64 with row stride ldt >= k, accumulation in float64, one
 *   rounding to float32; 1 <= k <= m <= 80; out must not alias X. */
#define NSVD_RITZ_BAD_PIVOT 1 /* a Cholesky pivot was not positive: S is numerically rank deficient */
#define NSVD_RITZ_SWEEP_CAP 2 /* the Jacobi sweep cap was reached before the off-diagonal threshold */
size_t nsvd_tsgram_f64_workspace_bytes(int n, int m);
int nsvd_tsgram_f64(const float* X, long ldx, const float* Y, long ldy, int n, int m, double* XtX, double* XtY, void* ws,
                    size_t ws_bytes, void* stream);
int nsvd_ritz_step_f64(const double* S, const double* A, const double* C, int m, double* theta, double* resid,
                       double* Q, double* T, int* status, void* stream);
int nsvd_ts_rotate(const float* X, long ldx, int n, int m, const double* T, int ldt, int k, float* out, long ldo,
                   void* stream);

/* ---- next row: the dense side of the truncated-SVD baseline of the kernel SVD operators ------------------------------
 * The top L <= 64 singular triplets of the empirical cross operator C = k(xs, ys) / sqrt(n_x n_y) come from a two-sided
 * block iteration on bases U (n_x, m), V (n_y, m), m <= 80, with P = C V and R = C^T U from ONE nsvd_rbf_apply_pair /
 * nsvd_dot_apply_pair call (neural_svd_amd/nystrom_svd.py drives the loop; nsvd_ts_rotate applies Tu and Tv). These are
 * the two pieces beside that product. NEW SYMBOLS ONLY: NSVD_ABI_VERSION stays 6.
 *
 * nsvd_tsgram3_f64: XtX = X^T X, XtY = X^T Y and YtY = Y^T Y, (m, m) float64 row-major, of X, Y (n, m) float32 with row
 *   strides ldx, ldy >= m (in floats), in one pass: each row tile of X and Y is staged once and feeds all three
 *   accumulations. All three outputs are required; X may be Y. Otherwise nsvd_tsgram_f64's conventions: products and
 *   sums in float64, rows split over workgroups by the same rule, partial matrices reduced in slice order by a second
 *   launch (no atomics: bit-reproducible), 1 <= m <= 80 (NSVD_EUNSUPPORTED above), any n >= 1, workspace 256-byte
 *   aligned, its size 0 for shapes outside these ranges.
 * nsvd_svd_ritz_step_f64: one workgroup, float64, everything (m, m) contiguous row-major. With
 *   Sp = P^T P, PtU = P^T U, Cu = U^T U, Sr = R^T R, RtV = R^T V, Cv = V^T V (two nsvd_tsgram3_f64 calls):
 *       Hl = PtU^T, Hr = RtV (both U^T C V up to the float32 rounding of P and R);
 *       H = (Hl + Hr) / 2 = A diag(sigma) B^T, sigma descending and >= 0, ties by ascending index (one-sided Jacobi on
 *       the columns of H in a fixed round-robin ordering: a pair is rotated when |g_p . g_q| > 1e-15 |g_p| |g_q|, a sweep
 *       without a rotation ends the loop, at most 40 sweeps; sigma_k = |g_k|, a_k = g_k / sigma_k - never through
 *       eigh(H^T H), which would square the trailing singular values into the rounding of the leading ones);
 *       Mp = B^T Sp B, Mr = A^T Sr A;
 *       resid_l_k = sqrt(max(Mp_kk - 2 sigma_k (A^T Hl B)_kk + sigma_k^2 (A^T Cu A)_kk, 0)) = |P b_k - sigma_k U a_k|,
 *       resid_r_k = sqrt(max(Mr_kk - 2 sigma_k (A^T Hr B)_kk + sigma_k^2 (B^T Cv B)_kk, 0)) = |R a_k - sigma_k V b_k|
 *       - identities for ANY U, A, B: the short form Mp_kk - sigma_k^2 assumes an orthonormal U and H = U^T P exactly, and
 *       with a float32 U and an H that averages two float32-derived matrices its square root stalls at 1e-4 sigma_0;
 *       Tu = B chol(Mp)^-1, Tv = A chol(Mr)^-1 (upper Cholesky factors): P Tu and R Tv are orthonormal bases of span(P)
 *       and span(R) whose leading columns are the Ritz directions in order.
 *   Cu / Cv NULL stand for the identity (the same bits as passing it). sigma, resid_l, resid_r, A, B may be NULL; Tu, Tv
 *   and status are required. *status (device int, zeroed by the caller) has NSVD_RITZ_* bits OR-ed in. On a
 *   non-positive (or non-finite) pivot that T is zero from the column on (NSVD_RITZ_BAD_PIVOT); sigma_k = 0 gives a zero
 *   column of A, never a division, and surfaces as a bad pivot of Mr. Nothing non-finite is ever stored. m > 80 is
 *   NSVD_EUNSUPPORTED; a NULL required pointer or m <= 0 is NSVD_EINVAL; a refused call writes nothing. Every loop of
 *   the kernel has a trip count bounded by m or a constant. Restated in float64 numpy by tests/_ksvd_oracle.py. */
size_t nsvd_tsgram3_f64_workspace_bytes(int n, int m);
int nsvd_tsgram3_f64(const float* X, long ldx, const float* Y, long ldy, int n, int m, double* XtX, double* XtY,
                     double* YtY, void* ws, size_t ws_bytes, void* stream);
int nsvd_svd_ritz_step_f64(const double* PtU, const double* RtV, const double* Sp, const double* Sr, const double* Cu,
                           const double* Cv, int m, double* sigma, double* resid_l, double* resid_r, double* A, double* B,
                           double* Tu, double* Tv, int* status, void* stream);

/* ---- next row: SpIN on the matrix-free kernel operators (methods/spin.py) ----------------------------------------------
 * The two pieces of SpIN's step that are its own; the moments come from nsvd_tsgram_f64, the term-1 cotangents
 * dphi = Kphi gpi / B1, dKphi = phi gpi / B1 (Covariance.backward, spin.py:76-100) from nsvd_ts_rotate, and the parameter
 * gradients of both from nsvd_model_backward (dKphi first through one more matrix-free product with the arguments
 * swapped: the kernels are symmetric). NEW SYMBOLS ONLY: NSVD_ABI_VERSION stays 6.
 *
 * nsvd_spin_solve (spin.py:33-38 spin_step, :41-59 SpINFunction.forward, :139-148 of _compute_loss): one workgroup,
 *   float64, everything (L, L) contiguous row-major, 2 <= L <= 64 (NSVD_EUNSUPPORTED above):
 *       sigma = sigma_scale * sigma_raw, pi = pi_scale * pi_raw  (the raw Gram matrices X^T X, X^T Y of nsvd_tsgram_f64)
 *       sigma_avg <- (1 - decay) sigma_avg + decay sigma          (float32 state, IN PLACE; zeros at the start, no bias
 *                                                                  correction; the solve uses the unrounded value)
 *       chol = cholesky(sigma_avg + 1e-3 I) (lower, float32 out), Ci = chol^-1, Lambda = Ci pi Ci^T
 *       loss_eigvals[0] = trace(Lambda), loss_eigvals[1 .. L] = diag(Lambda)
 *       gsigma = Ci^T triu(Lambda diag(diag Ci)), gpi_scaled = gpi_scale * (-Ci^T diag(diag Ci))   (float64 out)
 *   *status (device int, zeroed by the caller) has NSVD_RITZ_BAD_PIVOT OR-ed in on a non-positive or non-finite pivot
 *   or any non-finite result: chol, loss_eigvals, gsigma and gpi_scaled are then all zero and a non-finite element of
 *   sigma_avg is left as it was - nothing non-finite is stored. Every loop has a trip count bounded by L.
 *
 * nsvd_spin_jac_step (spin.py:15-30 jac_model_params, :155-167 of _compute_loss): for the plain model (no exponential
 *   or box mask: NSVD_EUNSUPPORTED; D <= 64, L <= 64, 1 .. NSVD_MAX_LAYERS layers of any width, B1 >= 2)
 *       j_new[a, c] = (2 / B1) sum_b phi[b, a] d model_c(x_b) / d p;   J <- (1 - decay) J + decay j_new;
 *       grads += sum_a gsigma[a, c] J[a, c]                            (ADDED: the caller zeroes or pre-fills grads)
 *   The reference's j_avg.<name> tensors (L, L, *p.shape) are zero outside head c's slice of index [a, c]; the state J
 *   keeps that slice alone: J[a], a < L, is one parameter set [W_0 | .. | W_n | b_0 | .. | b_n] (the nsvd_params layouts,
 *   contiguous, no padding) of nsvd_spin_state_floats floats, J[a][..][c][..] = j_avg[a, c, c, ..]. x (B1, D), phi (B1, L)
 *   = model(x) with the same hard_mul_const, gsigma (L, L) float64. Activations and unit-seed deltas are recomputed from
 *   x into `ws` (nsvd_spin_jac_workspace_bytes, 256-byte aligned; 0 for an unsupported description): no workspace of a
 *   model forward is needed. The contraction over b runs on v_mfma_f32_32x32x2_f32; sums over a are taken in ascending
 *   order (registers, then a fixed-order second launch): no atomics, bit-reproducible. */
int nsvd_spin_solve(const double* sigma_raw, double sigma_scale, const double* pi_raw, double pi_scale, int L,
                    double decay, double gpi_scale, float* sigma_avg, float* chol, double* loss_eigvals, double* gsigma,
                    double* gpi_scaled, int* status, void* stream);
size_t nsvd_spin_state_floats(const nsvd_model_desc* desc);
size_t nsvd_spin_jac_workspace_bytes(const nsvd_model_desc* desc, int B1);
int nsvd_spin_jac_step(const nsvd_model_desc* desc, const nsvd_params* params, const float* x, int B1, const float* phi,
                       float hard_mul_const, const double* gsigma, double decay, float* J, const nsvd_params* grads,
                       void* ws, size_t ws_bytes, void* stream);

/* ---- next row: SpINx on the matrix-free kernel operators (methods/spinx.py) --------------------------------------------
 * SpINx keeps SpIN's Cholesky whitening, drops the per-sample Jacobian contraction, differentiates straight through
 * cholesky(sigma + 1e-3 I) of the BATCH sigma and adds one squared-residual loss per eigenfunction. Its loss is a
 * function of four L x L moment matrices (nsvd_tsgram_f64 on all rows, nsvd_tsgram3_f64 on (P, K)); these are the two
 * pieces beside them. NEW SYMBOLS ONLY: NSVD_ABI_VERSION stays 6.
 *
 * nsvd_spinx_solve (spinx.py:13-23 SpINxLossFunction.forward with its autograd backward, :92-99 SpINx._compute_loss):
 *   one workgroup, float64, everything (L, L) contiguous row-major, 2 <= L <= 64 (NSVD_EUNSUPPORTED above). With
 *       S = s_scale S_raw (all rows), Gpp = g_scale Gpp_raw = P^T P / B1, Gpk = g_scale Gpk_raw = P^T K / B1 (= pi),
 *       Gkk = g_scale Gkk_raw = K^T K / B1 (S_raw and Gpp_raw may be one pointer), A = cholesky(S + 1e-3 I)^-1, rows a_l:
 *       lambda_l = a_l^T Gpk a_l, qk_l = a_l^T Gkk a_l, qp_l = a_l^T Gpp a_l
 *       losses = [sum_l trace_w_l lambda_l | qk_l - lambda_l^2 (2 - qp_l)]  (L + 1; the second part is
 *                mean_b (K a_l - lambda_l P a_l)^2 because Gpk is pi itself; trace_w NULL = ones)
 *       loss = sum_k w_k losses_k / L                                       (w: L + 1 float64 on the device)
 *       out64 = [loss | losses (L + 1) | lambda (L)]                         (2 L + 2 float64)
 *   and the reverse mode of loss, already scaled for the tall products (sigma_bar through the Cholesky factor):
 *       T_s = (S_bar + S_bar^T) s_scale,  T_pp = (Gpp_bar + Gpp_bar^T) g_scale + T_s,  T_kp = Gpk_bar^T g_scale,
 *       T_pk = Gpk_bar g_scale,  T_kk = (Gkk_bar + Gkk_bar^T) g_scale
 *   so that dP = P T_pp + K T_kp, dK = P T_pk + K T_kk (two nsvd_ts_rotate2 calls) and, with split rows, dPhi = Phi T_s
 *   on the rows that carry no K.
 *   update_state != 0: sigma_avg <- (1 - decay) sigma_avg + decay S (float32 state, IN PLACE, no bias correction) and
 *   chol = cholesky(sigma_avg + 1e-3 I) (lower, float32): a second factorisation, used only by SpINx.forward.
 *   update_state == 0: neither state tensor is read or written (both may be NULL).
 *   *status (device int, zeroed by the caller) has NSVD_RITZ_BAD_PIVOT OR-ed in on a non-positive or non-finite pivot
 *   of either factorisation or any non-finite result: out64, the five T's and (with update_state) chol are then all
 *   zero and a non-finite element of sigma_avg is left as it was - nothing non-finite is stored. Every loop has a trip
 *   count bounded by L. The Grams are read from global memory; no workspace.
 * nsvd_ts_rotate2: out (n, k) = X (n, m) T1[:, :k] + Y (n, m) T2[:, :k], X, Y float32 with row strides ldx, ldy >= m, T1, T2
 *   float64 with row strides ldt1, ldt2 >= k; both products and their sum accumulate in float64, one rounding to float32;
 *   1 <= k <= m <= 80; out must not alias X or Y (NSVD_EINVAL). */
int nsvd_spinx_solve(const double* S_raw, double s_scale, const double* Gpp_raw, const double* Gpk_raw,
                     const double* Gkk_raw, double g_scale, int L, const double* w, const double* trace_w, double decay,
                     int update_state, float* sigma_avg, float* chol, double* out64, double* T_s, double* T_pp,
                     double* T_kp, double* T_pk, double* T_kk, int* status, void* stream);
int nsvd_ts_rotate2(const float* X, long ldx, const float* Y, long ldy, int n, int m, const double* T1, int ldt1,
                    const double* T2, int ldt2, int k, float* out, long ldo, void* stream);

/* ---- next row: the CDK (two-tower) NestedLoRA loss ------------------------------------------------------
 * NestedLoRALossFunctionForCDK (methods/nestedlora.py:273-332) as called by NestedLoRAForCDK.compute_loss
 * (methods/nestedlora.py:366-378; examples/cdk/sketchy/main_sketchy.py:188).
 * f, g: (B, L) row-major float32 tower outputs. With Lp = L + (set_first_mode_const != 0):
 *   f~ = batch_weights[:, None] * [1, f]  (constant first mode when set_first_mode_const; weights optional, (B,))
 *   lam_f = f~^T f~ / B, lam_g = g~^T g~ / B
 *   loss[0] = loss[1] + loss[2]; loss[1] = -2 mean_b sum_l v_l f~ g~; loss[2] = sum(M * lam_f * lam_g)
 *   rs_joint (B) = diag(f~ g~^T), rs_indep (B (B-1)) = off_diagonal(f~ g~^T) (methods/utils.py:16-22); either
 *   may be NULL (both NULL skips the (B, B) gram contraction).
 * v: (Lp), M: (Lp, Lp) nesting masks (methods/nestedlora.py:345-359), float32 on the device.
 * ws: nsvd_cdk_workspace_bytes(B, L, set_first_mode_const) bytes, 256-byte aligned (NSVD_EINVAL otherwise, in the forward
 * and in the backward); keeps f~, g~ and M * lam for the backward.
 * Arithmetic is float32 on the fp32-input MFMA, independent of any autocast state of the caller. */
size_t nsvd_cdk_workspace_bytes(int B, int L, int set_first_mode_const);
int nsvd_cdk_loss_forward(const float* f, const float* g, const float* batch_weights, const float* v,
                          const float* M, int B, int L, int set_first_mode_const, float* loss, float* rs_joint,
                          float* rs_indep, void* ws, size_t ws_bytes, void* stream);

/* NestedLoRALossFunctionForCDK.backward (methods/nestedlora.py:309-332) after nsvd_cdk_loss_forward on the
 * same ws:  grad_f = grad_out * ( -(2/B) g~ v + (2/B) f~ (M * lam_g) )[:, first:], grad_g with f <-> g.
 * As in the reference the result is the gradient w.r.t. the WEIGHTED features (batch_weights are not
 * chain-ruled) and the constant column is dropped. grad_out: device scalar (the autograd grad_output, e.g.
 * the AMP loss scale) or NULL for 1. grad_f / grad_g: (B, L), either may be NULL. */
int nsvd_cdk_loss_backward(const float* v, int B, int L, int set_first_mode_const, const float* grad_out,
                           float* grad_f, float* grad_g, void* ws, size_t ws_bytes, void* stream);

/* normalize(z, r_up, regularize_mode) applied to the CDK towers' embeddings (examples/models/siam.py:170-183, called
 * from HeteroNetwork.forward_single :156-166). z, out, dout, dz: (B, L) float32 row-major.
 *   NSVD_NORMALIZE_L2_BALL:   rows with ||z|| < r_up unchanged, the others r_up * z / max(||z||, 1e-12)
 *   NSVD_NORMALIZE_L2_SPHERE: every row r_up * z / max(||z||, 1e-12)
 * Backward of the same expression (the comparison is a constant mask, as in the reference). out may alias z in the
 * forward; dz may alias dout in the backward. */
#define NSVD_NORMALIZE_L2_BALL 0
#define NSVD_NORMALIZE_L2_SPHERE 1
int nsvd_row_normalize_forward(const float* z, int B, int L, float r_up, int mode, float* out, void* stream);
int nsvd_row_normalize_backward(const float* z, const float* dout, int B, int L, float r_up, int mode, float* dz,
                                void* stream);

/* One CDK tower: Linear(d0 -> d1) -> BatchNorm1d(d1) -> LeakyReLU(slope) -> Linear(d1 -> d2) -> BatchNorm1d(d2), what
 * get_mlp(sizes=[d0, d1, d2], bias=True, nonlinearity='lrelu<slope>', use_bn=True) builds (examples/models/mlp.py:129-164)
 * and main_sketchy.py:107-116 uses as the two backbones of HeteroNetwork (examples/models/siam.py:132-166), in
 * TRAINING mode (batch statistics; running_mean / running_var updated with `momentum` when update_running != 0, as
 * torch.nn.BatchNorm1d does). Replaces the module's forward and its autograd backward. fp32 MFMA contractions.
 *   x (B, d0); z (B, d2); dz (B, d2); every parameter / gradient in torch's layout: W1 (d1, d0), b1 (d1), g1 / be1 /
 *   rm1 / rv1 (d1) = BatchNorm weight / bias / running_mean / running_var, W2 (d2, d1), b2, g2, be2, rm2, rv2 (d2).
 *   Shapes: B, d0, d1, d2 multiples of 128, B <= 1024 (anything else: NSVD_EINVAL; 0 from the size query).
 *   The forward leaves what the backward needs in `ws` (nsvd_tower_workspace_bytes): call the backward with the same
 *   x, parameters and workspace. The gradient w.r.t. x is not produced (the towers' inputs are data). */
typedef struct nsvd_tower_params {
    float *W1, *b1, *g1, *be1, *rm1, *rv1;
    float *W2, *b2, *g2, *be2, *rm2, *rv2;
} nsvd_tower_params;
size_t nsvd_tower_workspace_bytes(int B, int d0, int d1, int d2);
/*   gemm_bf16 != 0: MIXED PRECISION, the role of the reference's autocast branch (examples/cdk/sketchy/
 *   main_sketchy.py:161,182, on by default there: Linear and BatchNorm / activation outputs are half tensors, statistics
 *   and master weights float32) with bfloat16 as the half type and no GradScaler: X, W1, W2 are rounded to bfloat16
 *   (round to nearest even), the wide activations Y1 = X W1^T + b1, A1 = lrelu(BN1(Y1)) and the gradients dY2, dA1, dY1
 *   are STORED as bfloat16, the five contractions run on the bf16 MFMA with float32 accumulation (csrc/gemm16.h, no
 *   transposed copies), BatchNorm statistics, the narrow end (Y2, Z) and every parameter gradient stay float32.
 *   Not bit-comparable with float16 autocast; pinned to the float64 oracle with the same roundings. Shapes:
 *   nsvd_tower_mixed_supported (B, d1, d2 multiples of 256, d0 of 128, B <= 1024), NSVD_EUNSUPPORTED otherwise. The
 *   backward must be called with the flag of its forward (the workspace holds bfloat16 activations).
 *   Bit 1 (value 2) of the flag, forward only: the bfloat16 copies of W1 / W2 inside `ws` are current - set by callers
 *   that know the weights have not changed since the copies were written (nsvd_cdk_step's optimiser kernel refreshes
 *   them while it updates the float32 masters); clear, the forward casts the masters first. */
int nsvd_tower_mixed_supported(int B, int d0, int d1, int d2);
/*   Which of the two mixed-precision forms a call with this shape and activation slope runs. 1: the wide layer with
 *   BatchNorm INSIDE the contraction (csrc/tower_col.h, slope > 0): Y1 and dA1 stay float32 in the accumulators and are
 *   never stored (statistics, normalisation and the activation on unrounded values); the backward recovers the normalised
 *   value from the stored bfloat16 activation, h = A1 > 0 ? A1 : A1 / slope, yhat = (h - beta1) / gamma1 (needs
 *   gamma1 != 0). 0: contraction + strip kernels, Y1 and dA1 stored as bfloat16 as described above (slope == 0: ReLU is
 *   not invertible). The float64 oracle restates both (oracle.tower_forward_backward: gemm_bf16 = "fused" / True). */
int nsvd_tower_mixed_fused(int B, int d0, int d1, int d2, float slope);
int nsvd_tower_forward(const float* x, const nsvd_tower_params* params, int B, int d0, int d1, int d2, float slope,
                       float eps, float momentum, int update_running, int gemm_bf16, float* z, void* ws,
                       size_t ws_bytes, void* stream);
int nsvd_tower_backward(const float* x, const nsvd_tower_params* params, const float* dz, int B, int d0, int d1,
                        int d2, float slope, int gemm_bf16, const nsvd_tower_params* grads, void* ws, size_t ws_bytes,
                        void* stream);
/* A tower whose HIDDEN width is sharded over processes (rank r holds rows [r d1/W, (r+1) d1/W) of W1, b1 and the
 * first BatchNorm, and the same columns of W2; b2 and the second BatchNorm are replicated): d1 is the LOCAL width.
 * BatchNorm statistics are per column, so the first half needs no exchange and the arithmetic is the unsharded tower's
 * (the reference's is single-process: examples/models/mlp.py:129-164). phase 1: Linear1, BatchNorm1, activation and this
 * rank's PARTIAL product A1 W2^T (no bias) into the workspace at nsvd_tower_y2_offset - (B, d2) floats the caller sums
 * over the ranks in place (one all-reduce); phase 2: + b2, BatchNorm2 -> z. phase 0 = nsvd_tower_forward. The
 * backward (nsvd_tower_backward with the local d1) needs no exchange: dz is replicated, every other quantity local. */
size_t nsvd_tower_y2_offset(int B, int d0, int d1, int d2);
int nsvd_tower_forward_phase(const float* x, const nsvd_tower_params* params, int B, int d0, int d1, int d2,
                             float slope, float eps, float momentum, int update_running, int gemm_bf16, int phase,
                             float* z, void* ws, size_t ws_bytes, void* stream);

/* nsvd_operator_backward_evd_step for the heads [l_begin, l_begin + l_count) only: ONE fused step taken as several head
 * windows (the heads of ParallelMLP share nothing but the input, examples/models/mlp.py:187-189), each window its own
 * pair of launches, possibly on its own stream - a two-window step lets the latency-bound chain of window 1 and the
 * HBM-bound optimiser epilogue of window 0 sit under the other window's MFMA loops (trainer.FusedTrainer
 * (backward_windows=2)). Every window of a step gets the same arguments except l_begin / l_count, last_window and
 * ev_after_chain; the windows must cover every head exactly once; last_window != 0 on exactly one of them, the one whose
 * launches are ordered behind the CHAIN launches of all others: it advances the device-resident schedule (opt->state)
 * and adds up the loss scalars. ev_after_chain: NULL, or a hipEvent_t this call records between its two launches (what
 * the next window's stream waits for). x_next != NULL (one window of the step only): the next batch is drawn and its
 * features written by guest workgroups of this window's first launch, as nsvd_operator_backward_evd_step_next does.
 * Fused MFMA path, windows whose weight-gradient contraction needs no batch slices
 * (nsvd_backward_head_window_ok), direct or reduced moments: NSVD_EUNSUPPORTED otherwise. Results are bit-identical to
 * the one-call step. */
int nsvd_operator_backward_evd_step_window(const nsvd_model_desc* desc, const nsvd_params* params,
                                           const nsvd_problem* prob, const float* x, int B, const float* f,
                                           const float* Tf, int mask_kind, const float* v, const float* M,
                                           float* moments, int moments_reduced, const void* evd_scratch, int L_total,
                                           int l_offset, float grad_scale, float* loss, const nsvd_params* grads,
                                           const nsvd_rmsprop* opt, void* ws, size_t ws_bytes, int path, int l_begin,
                                           int l_count, int last_window, void* ev_after_chain,
                                           unsigned long long next_seed, unsigned long long next_offset, float* x_next,
                                           void* ws_next, size_t ws_next_bytes, void* stream);

/* nsvd_operator_backward_evd_step that ALSO draws the next batch and writes its Fourier features - what
 * nsvd_operator_sample_features(next_seed, next_offset, x_next, ws_next) does as a launch of its own - as guest
 * workgroups of the backward's first kernel: sampling and features (main_pde.py:92-93, examples/utils.py:139-140)
 * depend on no weight, and that kernel's own workgroups are latency-bound, so the feature launch of the next step and
 * its kernel boundary disappear. ws_next: a second workspace of nsvd_workspace_bytes(desc, B) bytes, distinct from ws;
 * the next nsvd_operator_forward is then called on (x_next, ws_next) with NSVD_FEATURES_READY. MFMA path only
 * (NSVD_EUNSUPPORTED otherwise: call the two entry points separately). Results are bit-identical to the separate calls. */
int nsvd_operator_backward_evd_step_next(const nsvd_model_desc* desc, const nsvd_params* params,
                                         const nsvd_problem* prob, const float* x, int B, const float* f,
                                         const float* Tf, int mask_kind, const float* v, const float* M,
                                         float* moments, int moments_reduced, const void* evd_scratch, int L_total,
                                         int l_offset, float grad_scale, float* loss, const nsvd_params* grads,
                                         const nsvd_rmsprop* opt, void* ws, size_t ws_bytes, int path,
                                         unsigned long long next_seed, unsigned long long next_offset, float* x_next,
                                         void* ws_next, size_t ws_next_bytes, void* stream);

/* The kernel-operator training step's backward half in one call (NestedLoRA.compute_loss_kernel with
 * split_batch = False, methods/nestedlora.py:230-252, followed by loss.backward(); optimizer.step(); ema.update()):
 * after nsvd_model_forward(save_for_backward = 1) produced f = model(x) and the caller computed Tf = Kf from it
 * (nsvd_kernel_apply; no gradient flows through Kf: NestedLoRALossFunctionEVD.backward, methods/nestedlora.py:98-111),
 * this evaluates d loss / d f per sample inside the backward kernels from the moments (as
 * nsvd_operator_backward_evd does: same `moments` / `moments_reduced` / `evd_scratch` conventions), runs autograd's
 * backward of the plain model evaluation and - when opt != NULL - takes the RMSprop (+ EMA) step in the epilogue of
 * the weight-gradient kernel (grads may then be NULL). L_total / l_offset as in nsvd_operator_backward_evd: desc
 * describes the heads [l_offset, l_offset + desc->L) of a model of L_total heads whose f, Tf (B, L_total), moments and
 * masks are global (heads sharded over processes); 0, 0 = all heads. Input dimension up to 64; MFMA path only
 * (128-wide hidden layers, B a multiple of 32): NSVD_EUNSUPPORTED otherwise. ws: the workspace of the
 * nsvd_model_forward call. */
int nsvd_model_backward_evd_step(const nsvd_model_desc* desc, const nsvd_params* params, const float* x, int B,
                                 const float* f, const float* Tf, int mask_kind, const float* v, const float* M,
                                 float* moments, int moments_reduced, const void* evd_scratch, int L_total,
                                 int l_offset, float grad_scale, float* loss, const nsvd_params* grads,
                                 const nsvd_rmsprop* opt, void* ws, size_t ws_bytes, void* stream);

/* One Sketchy-style CDK training step in ONE call: the loop body of examples/cdk/sketchy/main_sketchy.py:180-212 as
 * scripts/exps/sketchy.sh configures it (sgd, momentum 0.9, --clip_grad_norm), AMP branches off:
 *     optimizer.zero_grad(); _, fx, _, fy = method(x, y); loss, *_ = method.compute_loss(fx, fy); loss.backward()
 *     nn.utils.clip_grad_norm_(model.parameters(), max_norm); optimizer.step()
 * with model = HeteroNetwork(two get_mlp towers, Identity projectors, mu, regularize_mode) (examples/models/siam.py:132-166)
 * and method = NestedLoRAForCDK(model, neigs = d2, ...) (methods/nestedlora.py:335-378). Stages: nsvd_tower_forward x 2
 * (running statistics updated), nsvd_row_normalize_forward x 2 (radius sqrt(mu)), nsvd_cdk_loss_forward / _backward,
 * nsvd_row_normalize_backward x 2, nsvd_tower_backward x 2, then the total gradient norm over all 16 parameter tensors
 * in a fixed summation order, torch's clip coefficient min(1, max_grad_norm / (norm + 1e-6)) (max_grad_norm <= 0: no
 * clipping) and torch.optim.SGD's momentum update (no dampening, nesterov or weight decay):
 *     g <- coef g;  buf <- g (first_step) or momentum buf + g;  p <- p - lr buf
 * towers[2] (x tower, y tower): parameters and running statistics, UPDATED IN PLACE; momentum_bufs[2]: the optimiser's
 * momentum buffers in the same layouts (rm / rv fields unused). lr is the already scheduled value. x, y: (B, d0).
 * v (d2 + first), M ((d2 + first)^2): nesting masks. loss[0..3] = {loss, operator term, metric term, total gradient
 * norm before clipping}. rs_joint (B) / rs_indep (B (B - 1)): the loss's diagnostics, or NULL. Shapes as for
 * nsvd_tower_forward. ws: nsvd_cdk_step_workspace_bytes (0 for an unsupported description). */
typedef struct nsvd_cdk_step_desc {
    int32_t B, d0, d1, d2;
    float slope, bn_eps, bn_momentum;
    float mu;
    int32_t normalize_mode;       /* NSVD_NORMALIZE_* */
    int32_t set_first_mode_const;
    double lr, momentum, max_grad_norm;
    int32_t first_step;
    int32_t gemm_bf16;            /* != 0: the towers in mixed precision (nsvd_tower_forward; bit 1: this workspace's
                                   * bfloat16 weight copies are those the previous nsvd_cdk_step call left; bit 4,
                                   * value 16: the half type is IEEE float16 instead of bfloat16) */
    int32_t reserved0;
    void* grad_scaler;            /* NULL, or a DEVICE nsvd_grad_scaler: the step runs with loss scaling (below) */
} nsvd_cdk_step_desc;
/* torch.cuda.amp.GradScaler's state and arithmetic on the device - the reference's AMP branch, on by default in the
 * Sketchy script (examples/cdk/sketchy/main_sketchy.py:161 scaler = GradScaler(enabled=use_amp); :194-208
 * scaler.scale(loss).backward(); scaler.unscale_(optimizer); clip_grad_norm_; scaler.step(optimizer); scaler.update();
 * lr_scheduler.step() on EVERY iteration, skipped or not, :205-206 - this script has no scheduler gate, unlike the PDE
 * loop's examples/operator/__init__.py:66-72: desc.lr stays the caller's scheduled value of the iteration). With
 * desc.grad_scaler set, nsvd_cdk_step
 *   - multiplies the loss gradient by `scale` where the backward starts (every stored 16-bit gradient is scaled),
 *   - takes found_inf = the gradient norm (of the scaled gradients, float32) is not finite,
 *   - found_inf: NO parameter, momentum buffer or weight copy is written (scaler.step skips optimizer.step()), scale *=
 *     backoff_factor, growth_tracker = 0, steps_skipped += 1;
 *   - otherwise: gradients * (1 / scale), then the clip coefficient and the SGD update as without scaling; steps_ok += 1,
 *     growth_tracker += 1 and at growth_interval: scale *= growth_factor, growth_tracker = 0 (GradScaler.update()).
 *   desc.first_step is ignored: the momentum buffers start with the first step TAKEN (steps_ok == 0), as torch.optim.SGD
 *   creates them in its first executed step().
 * The loss values reported are unscaled. Needs the mixed-precision step with the fused narrow end (cdk_narrow.hip:
 * B % 8 == 0, d2 <= 1024 and d2 / 4 dividing 256 - with the mixed-precision rule d2 % 256 == 0: d2 in {256, 512, 1024}),
 * NSVD_EUNSUPPORTED otherwise. Read the state back with a device-to-host copy. */
typedef struct nsvd_grad_scaler {
    float scale;
    float growth_factor;      /* torch default 2 */
    float backoff_factor;     /* 0.5 */
    int32_t growth_interval;  /* 2000 */
    int32_t growth_tracker;
    int32_t steps_ok;
    int32_t steps_skipped;
    int32_t last_found_inf;
} nsvd_grad_scaler;
int nsvd_grad_scaler_init(void* state, float init_scale, float growth_factor, float backoff_factor, int growth_interval,
                          void* stream);
size_t nsvd_cdk_step_workspace_bytes(const nsvd_cdk_step_desc* desc);
int nsvd_cdk_step(const nsvd_cdk_step_desc* desc, const float* x, const float* y, const nsvd_tower_params* towers,
                  const nsvd_tower_params* momentum_bufs, const float* v, const float* M, float* loss,
                  float* rs_joint, float* rs_indep, void* ws, size_t ws_bytes, void* stream);

/* C = A B^T on the bf16 MFMA, float32 accumulation: the contraction of the mixed-precision towers (csrc/gemm16.h) as an
 * entry point of its own - what torch.matmul on bfloat16 tensors is to the reference's autocast branch
 * (examples/cdk/sketchy/main_sketchy.py:182; the reference's half type is float16). A, B hold bfloat16 values.
 *   a_kstrided == 0: A is (M, lda), row m = the K contraction values of output row m (contiguous)
 *   a_kstrided != 0: A is (K, lda), row k = the M values of contraction index k (A^T as stored: no transposed copy)
 *   likewise B / b_kstrided with N columns of C. (A strided with B contiguous is not built.)
 * C (M, ldc): float32, or bfloat16 when out_bf16; bias (N) is added per column when not NULL. slices > 1: split-K,
 * slice s contracts k in [s K / slices, (s + 1) K / slices) into C + s * slice_stride (elements; bias goes to every
 * slice: pass NULL). sumsq: NULL, or (M / 256) (N / 128) slices floats - per tile, the sum of squares of the
 * float32 values BEFORE any bfloat16 rounding of the store (the gradient norm is taken of the float32 gradient).
 * M % 256 == 0, N % 128 == 0, K % (64 slices) == 0, lda, ldb % 8 == 0, ldc % 4 == 0, 16-byte aligned pointers. */
int nsvd_gemm_bf16(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long lda, long ldb,
                   long ldc, int a_kstrided, int b_kstrided, int out_bf16, int slices, long slice_stride, float* sumsq,
                   void* stream);
/* out[i] = bfloat16(in[i]) (round to nearest even), n % 8 == 0, 16-byte aligned pointers */
int nsvd_to_bf16(const float* in, void* out, size_t n, void* stream);

/* ---- NeuralEF (mu-EigenGame) on the operator path: methods/neuralef.py, methods/utils.py:36-68 ------------------
 * nsvd_nef_operator_forward: Tphi, phi = operator(BatchL2NormalizedFunctions(model), x, importance) in training mode
 * (neuralef.py:139-152 -> diff_ops.py:25-52). Each of the 1 + 2D stencil points is divided by its own per-head batch
 * norm n_e = ||u_e[:, l]|| / sqrt(B) of the WaveFunctions output u_e (utils.py:48-56); the shifted norms come from the
 * even / odd rows (n_e^2 - n_0^2 formed per sample) and 1 / n_e is folded into the even / odd stencil. The running
 * norms norm_biased / norm_unbiased (1, L) take 1 + 2D updates in stencil order (utils.py:58-68); *initialized == 0
 * makes the first one a copy, and the call sets it to 1 (device int, so a step can be captured in a graph).
 * Outputs phi, Tphi (B, L), and for nsvd_nef_operator_backward: h = u0 / n0, r = sqrt p / clamp(sqrt p, 1e-5) (B, L),
 * stats ((1 + 2D) L: n0, then n0 / n_e - 1 per shifted point). ws: as for nsvd_operator_forward (always saved for the
 * backward). Float32 stencil paths only (PATH_AUTO / FUSED / GENERIC; eps > 0). */
int nsvd_nef_operator_forward(const nsvd_model_desc* desc, const nsvd_params* params, const nsvd_problem* prob,
                              const float* x, int B, float* phi, float* Tphi, float* h, float* r, float* stats,
                              float* norm_biased, float* norm_unbiased, int* initialized, float momentum, void* ws,
                              size_t ws_bytes, int path, void* stream);

/* Parameter gradients of sum(dphi * phi) through the centre evaluation and its batch normalisation (Tphi gets no
 * gradient, neuralef.py:61-62): du0 = (dh - h mean_b(dh h)) / n0 with dh = r dphi, then nsvd_operator_backward's centre
 * backward on du0 (du0: (B, L) scratch). Gradients are OVERWRITTEN. */
int nsvd_nef_operator_backward(const nsvd_model_desc* desc, const nsvd_params* params, const nsvd_problem* prob,
                               const float* x, int B, const float* dphi, const float* h, const float* r,
                               const float* stats, float* du0, const nsvd_params* grads, void* ws, size_t ws_bytes,
                               int path, void* stream);

/* NeuralEigenfunctionsLossFunction (methods/neuralef.py:13-62): loss[0] and d loss / d phi. variance = -Tphi / B;
 * unbiased: coeff_h = triu(phi_h^T phi_h / B_h, diagonal); biased: coeff_1 = triu(Q_2, diagonal) / (diag(Q_2) + 1e-5)
 * by row, Q_h = phi_h^T Tphi_h / B_h (each half the other's); align_h = Tphi_h coeff_h / B_h;
 * loss = sum(phi variance) + (sum(phi1 align_1) + sum(phi2 align_2)) / 2. phi1 / phi2 the two chunks of phi (B1 =
 * ceil(B / 2)): dphi = 4 variance + 2 align_h by rows (dphi1 / dphi2 unused); otherwise independent halves: dphi = 4
 * variance, dphi1 = 2 align_1, dphi2 = 2 align_2. The incoming gradient is ignored, as in the reference. L <= 64. */
size_t nsvd_nef_loss_workspace_bytes(int B, int B1, int B2, int L);
int nsvd_nef_loss(const float* phi, const float* Tphi, int B, const float* phi1, const float* Tphi1, int B1,
                  const float* phi2, const float* Tphi2, int B2, int L, int unbiased, int diagonal, float* loss,
                  float* dphi, float* dphi1, float* dphi2, void* scratch, size_t scratch_bytes, void* stream);

/* f[b, l] /= norm[l], Tf[b, l] /= norm[l] in place: BatchL2NormalizedFunctions in evaluation mode (utils.py:54-56). */
int nsvd_nef_scale_heads(float* f, float* Tf, const float* norm, int B, int L, void* stream);

/* ---- NeuralEF on a matrix-free kernel operator: the batch normalisation of a plain (B, L) block ---------------------
 * nsvd_nef_rows_forward: BatchL2NormalizedFunctions.forward in training mode (methods/utils.py:48-68) on the raw head
 * outputs u (B, L) of ONE model evaluation. The rows are one segment (B1 == B) or the two segments [0, B1) and [B1, B)
 * (the two model calls of a split step, methods/neuralef.py:113-118), each with at least one row. Per segment h and
 * head l: n_h[l] = ||u_h[:, l]|| / sqrt(B_h) (utils.py:51), phi = u / n_h (utils.py:56; phi may alias u), and stats
 * (2 L) = n_1 | n_2 (one segment: n_1 twice). A zero norm is divided by, as in the reference.
 * The running norms norm_biased / norm_unbiased (L each) take n_order <= 4 updates (utils.py:58-68), update k with the
 * norm of segment order[k] (a HOST array, read before the call returns): biased m r + (1 - m) n, unbiased
 * sqrt(m r^2 + (1 - m) n^2); *initialized == 0 makes the first one a copy, and a call with n_order > 0 sets it to 1
 * (device int: no host read in a step). n_order == 0 touches neither the running norms nor *initialized (all three
 * may then be NULL).
 * The column sums of squares are float64: per block of rows, then over the blocks by every workgroup that needs them,
 * each in a fixed order (no floating-point atomics: equal bits from run to run). 1 <= L <= 64, B <= 65536.
 * ws: nsvd_nef_rows_workspace_bytes(B, L) bytes (0: unsupported shape), 256-byte aligned.
 *
 * nsvd_nef_rows_backward: the cotangent of u. g = dphi (+ dphi1 + dphi2 when BOTH are given: the three gradients
 * NeuralEigenfunctionsLossFunction returns for phi1 = phi2 = phi, neuralef.py:61-62; each (B, L), added in float64),
 * s_h[l] = mean over the rows of segment h of g phi (float64, the same two ordered passes), du = (g - phi s_h) / n_h
 * formed in float64 and rounded once. du may alias dphi. stats == NULL (batchnorm_mode 'none'): du = g, phi unused. */
size_t nsvd_nef_rows_workspace_bytes(int B, int L);
int nsvd_nef_rows_forward(const float* u, int B, int B1, int L, float* phi, float* stats, float* norm_biased,
                          float* norm_unbiased, int* initialized, float momentum, const int* order, int n_order,
                          void* ws, size_t ws_bytes, void* stream);
int nsvd_nef_rows_backward(const float* phi, const float* stats, int B, int B1, int L, const float* dphi,
                           const float* dphi1, const float* dphi2, float* du, void* ws, size_t ws_bytes, void* stream);

/* ---- Retrieval metrics of the CDK towers: examples/cdk/sketchy/retrieve.py ----------------------------------------
 * For each of the Nq queries the WHOLE gallery is ranked by descending key, ties by ASCENDING gallery index (a stable
 * sort; faiss leaves ties open, here the rule is part of the contract). Key s_ij: NSVD_RETR_INNER_PRODUCT x_i . y_j
 * (IndexFlatIP), NSVD_RETR_EUCLIDEAN x_i . y_j - |y_j|^2 / 2 (the order of ascending |x_i - y_j|^2), float32 on the
 * fp32-input MFMA. zq (Nq, d), zg (Ng, d): float32 rows with leading dimensions ldq, ldg >= d, 4-byte aligned - a
 * truncation of an embedding is the window (z + col0, ld, d), no copy. 1 <= d <= nsvd_retrieval_max_d(),
 * 1 <= K <= min(Ng, nsvd_retrieval_max_k()), Ng <= nsvd_retrieval_max_gallery() (else NSVD_EUNSUPPORTED); Nq = 0 launches nothing.
 * With rel_j = (g_cls[j] == q_cls[i]), r_1 < ... < r_R the 1-based ranks of the relevant rows, p_m = m / r_m:
 *   topk_idx / topk_rel (Nq, K): gallery index at rank k + 1 and its relevance (either may be NULL);
 *   prec_at_k (Nq): #{m : r_m <= K} / K; hits_at_k (Nq) or NULL: that count itself;
 *   avg_prec (3, Nq) FLOAT64 or NULL - compute_average_precisions over the whole ranking: ver 1 = sum_m max_{m' >= m} p_m' / R,
 *     ver 2 = sum_m p_m / min(Ng, n_relevant_items[i]), ver 3 = sum_m p_m / R (float64 sums; R = 0: NaN, 0 / n, NaN);
 *   n_relevant_found (Nq) or NULL: R.
 * n_relevant_items (Nq) is an INPUT (the reference counts the query's class among the queries); needed with avg_prec.
 * ws: nsvd_retrieval_workspace_bytes(Nq, Ng, d, K) bytes (0: invalid description), 256-byte aligned; it holds one
 * chunk of query rows (about 64 MiB, at least 64 rows), never Nq x Ng. No atomics: bit-identical from run to run;
 * no allocation, synchronisation or read-back: capturable in a graph. */
#define NSVD_RETR_INNER_PRODUCT 0
#define NSVD_RETR_EUCLIDEAN 1
int nsvd_retrieval_max_gallery(void);
int nsvd_retrieval_max_k(void); /* 2048 */
int nsvd_retrieval_max_d(void); /* 1024 */
size_t nsvd_retrieval_workspace_bytes(int Nq, int Ng, int d, int K);
int nsvd_retrieval_eval(const float* zq, long ldq, const float* zg, long ldg, int Nq, int Ng, int d,
                        const int32_t* q_cls, const int32_t* g_cls, const int32_t* n_relevant_items, int metric, int K,
                        int32_t* topk_idx, uint8_t* topk_rel, float* prec_at_k, int32_t* hits_at_k, double* avg_prec,
                        int32_t* n_relevant_found, void* ws, size_t ws_bytes, void* stream);

/* Measurement aid (bench.py): record the two hipEvent_t handles immediately before / after the
 * DOMINANT kernel of the next nsvd_operator_forward call made by this host thread (the fused MFMA
 * forward kernel, or the layer-0 GEMM on the generic path), on that call's stream - or, whichever
 * comes first, around the first contraction (X W1^T) of the next nsvd_tower_forward / the gathered-row
 * contraction of the next nsvd_kernel_apply / the main kernel of the next nsvd_rbf_apply. One-shot; pass NULLs to clear. Per-thread state; the
 * compute entry points themselves stay stateless. */
int nsvd_profile_next_forward(void* ev_start, void* ev_stop);

#ifdef __cplusplus
}
#endif
#endif /* NSVD_H */
