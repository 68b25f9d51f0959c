/*
 * mile_hip.h -- C ABI of the MI355X-native MCLMC / NUTS ensemble sampler (libmile_hip.so).
 *
 * This is the drop-in boundary for ONE path of zhiyuan-yang/MILE: the MCLMC and
 * NUTS integrator steps over an ensemble of BNN-parameter particles with the
 * per-particle full-batch grad-log-posterior of the FCN MLP.  Every entry point
 * names the reference interface it replaces (paths relative to the reference
 * repository root).  The reference binds that path through Python callables
 * (blackjax.mclmc(logdensity_fn, L, step_size) -> SamplingAlgorithm(init, step));
 * a Python closure cannot cross a C ABI, so the closure's CONTENT crosses
 * instead: the model spec (src/config/models/fcn.py:7-30), the prior
 * (src/training/priors.py:67-91), the task (src/training/probabilistic.py:92-109)
 * and the training data (src/training/trainer.py:576-580).
 *
 * Conventions
 *   - All array pointers are DEVICE pointers into caller-owned memory (PyTorch-ROCm
 *     tensors), contiguous, row-major, fp32 unless stated.  The library never
 *     frees or retains caller memory beyond the call, except mile_set_data which
 *     COPIES X and y into its own padded layout, and mile_set_embedding, which COPIES
 *     the frozen embedding tables.
 *   - [E, d] arrays: one row per particle (chain), d = mile_param_count(), in
 *     jax.flatten_util.ravel_pytree order of the FCN param tree: for each layer in
 *     sorted-name order ('layer0','layer1','layer10','layer11','layer2',...):
 *     bias[out] then kernel[in, out] row-major (src/training/priors.py:105,
 *     src/training/warmup.py:341,442).
 *   - `stream` is a hipStream_t passed as void*; work is enqueued on it and the
 *     call returns without synchronising.  No internal threads.
 *   - Return value: 0 on success, negative mile_status on error; the message is
 *     available from mile_last_error() (thread-local).
 *   - One handle per device; a handle is not thread-safe; distinct handles are
 *     independent.
 */
#ifndef MILE_HIP_H_
#define MILE_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MILE_ABI_VERSION 10
#define MILE_MAX_LAYERS 16

typedef enum mile_status {
  MILE_OK = 0,
  MILE_ERR_INVALID = -1,     /* bad argument / unsupported spec */
  MILE_ERR_STATE = -2,       /* call order (e.g. no data set, workspace too small) */
  MILE_ERR_HIP = -3,         /* HIP runtime error */
  MILE_ERR_NOMEM = -4
} mile_status;

/* src/config/models/base.py:25-39 (Activation) */
typedef enum mile_activation { MILE_ACT_RELU = 0, MILE_ACT_TANH = 1, MILE_ACT_SIGMOID = 2 } mile_activation;
/* src/config/data.py Task; likelihoods at src/training/probabilistic.py:92-109 */
typedef enum mile_task { MILE_TASK_REGRESSION = 0, MILE_TASK_CLASSIFICATION = 1 } mile_task;
/* src/training/priors.py:47-49 (StandardNormal == NORMAL with loc 0, scale 1) */
typedef enum mile_prior { MILE_PRIOR_NORMAL = 0, MILE_PRIOR_LAPLACE = 1 } mile_prior;
/* Placement of the partial momentum refresh inside one kernel step. */
typedef enum mile_refresh { MILE_REFRESH_O_STEP_O = 0, MILE_REFRESH_STEP_O = 1 } mile_refresh;
/* Which grad-log-posterior kernel to use.  AUTO picks the fastest fp32-accurate kernel that supports the spec
 * (MFMA_W64_BF16X3 reproduces fp32 products exactly from three-term bf16 splits and counts as one); the
 * bf16-operand kernel MFMA_W128_BF16 (operands ROUNDED to bf16, fp32 accumulate) is only ever selected explicitly. */
typedef enum mile_grad_kernel {
  MILE_GRAD_AUTO = 0,
  MILE_GRAD_GENERIC = 1,          /* any FCN, fp32 VALU */
  MILE_GRAD_MFMA_W64 = 2,         /* ReLU regression, 1-3 hidden layers of width 64, fp32 MFMA */
  MILE_GRAD_MFMA_W128_BF16 = 3,   /* ReLU regression, 1-3 hidden layers of width 128, bf16 MFMA */
  MILE_GRAD_GEMM_F32 = 4,         /* any FCN, fp32: rocBLAS strided-batched SGEMMs + elementwise HIP kernels (wide nets) */
  MILE_GRAD_LENET_F32 = 5,        /* MILE_MODEL_LENET only: im2col + the same SGEMMs, pooling / col2im HIP kernels */
  MILE_GRAD_MFMA_W64_BF16X3 = 6,  /* as MFMA_W64 with 2-3 hidden layers; the hidden->hidden forward / dH / dW products run as six
                                     bf16 MFMA products of exact three-term bf16 splits of the fp32 operands (fp32-faithful) */
  MILE_GRAD_MFMA_WIDE_BF16X3 = 7, /* any FCN, layer-wise: hand-written batched MFMA GEMMs (k_mm3) with the same fp32-faithful
                                     three-term bf16 products, bias / activation / activation-derivative fused into their
                                     epilogues; what AUTO picks for wide nets (hidden width >= 96: B4's 4 x 256 softmax net) */
  MILE_GRAD_MFMA_WIDE_BF16 = 8,   /* the same kernels with bf16-ROUNDED operands (one product instead of six); explicit only */
  MILE_GRAD_MFMA_NARROW_F32 = 10, /* FCNs with 1-3 hidden layers of width <= 64, F <= 64 inputs (or 4-10 hidden layers of width <= 16,
                                     F <= 16: the reference's depth ablations), <= 16 outputs, any activation,
                                     either head: fused forward + backward on v_mfma_f32_16x16x4_f32 (fp32 operands -- exact fp32
                                     products, fp32 accumulation); what AUTO picks for the reference's own 16- / 32-wide nets
                                     (experiments/replicate_uci/mclmc.yaml [16,16,2], tabluar_classif/covertype.yaml [32,7]) */
  MILE_GRAD_LENET_BF16 = 9,       /* MILE_MODEL_LENET, <= 4 image channels: the five convolution products as implicit GEMMs on
                                     v_mfma_f32_16x16x32_bf16 with bf16-ROUNDED operands (BASELINE config 5 names bf16), the rest
                                     as LENET_F32; explicit only */
  MILE_GRAD_LENETTI_F32 = 11,     /* MILE_MODEL_LENETTI only (and its only kernel; AUTO resolves to it): one fused fp32 forward +
                                     backward launch, k_grad_lenetti (mile_lenetti.h); <= 4 image channels, (H+2)(W+2) <= 2048,
                                     out_dim <= 16 */
  MILE_GRAD_ATTN_F32 = 12,        /* MILE_MODEL_ATTN only (and its only kernel; AUTO resolves to it): one fused fp32 forward +
                                     backward launch, k_grad_attn (mile_attn.h), products on v_mfma_f32_16x16x4_f32; T <= 128,
                                     C <= 64, D <= 64 with H | D, <= 2 projections of width <= 64, n_classes <= 16, and
                                     <= 160 KB of LDS per workgroup (refused otherwise: H = 3, D in {57, 60, 63} with
                                     T > 112) */
  MILE_GRAD_ATTN_PRE_F32 = 13,    /* MILE_MODEL_ATTN_PRETRAINED only (and its only kernel; AUTO resolves to it): one fused fp32
                                     forward + backward launch, k_grad_attn_pre (mile_attn_pre.h), products on
                                     v_mfma_f32_16x16x4_f32, weights streamed from L2, gradients accumulated in the
                                     workgroup's own slab row; T <= 128, C <= 192, D <= 128 with H | D, <= 2 projections of
                                     width <= 128, n_classes <= 16, and <= 160 KB of LDS per workgroup (q|k|v [Tp][3D] + e
                                     [Tp][C] + vectors: e.g. C = 192, D = 64 needs T <= 96) */
  MILE_GRAD_ATTN_WIDE_F32 = 14,   /* MILE_MODEL_ATTN_WIDE only (and its only kernel; AUTO resolves to it): k_grad_attn_wide
                                     (mile_attn_wide.h), the ATTN_PRE_F32 kernel with the tables read from the chain's own
                                     parameters and their gradient added (dPos by owner threads, dEmb by fp32 vector atomics
                                     into the slab row's own [V][C] block); the same envelope and LDS as ATTN_PRE_F32.  Its
                                     row ranges are sized for that block (4 V C bytes per slab row), see mile_reserve */
  MILE_GRAD_LENET_BF16X3 = 15     /* MILE_MODEL_LENET, <= 4 image channels: LENET_BF16 with its five convolution products made
                                     fp32-faithful -- input, dZ and kernel operands as exact three-term bf16 splits (three term
                                     planes per LDS tile), six v_mfma_f32_16x16x32_bf16 products per accumulator, smallest first;
                                     the error against fp64 of the fp32 kernels and no library kernel.  Images whose three
                                     planes do not fit 150 KB of LDS are refused at the first gradient; explicit only */
} mile_grad_kernel;
/* Which network: the FCN (src/models/tabular/fcn.py:16-28), LeNet (src/models/images/cnns.py:10-66), LeNetti
 * (src/models/images/cnns.py:69-121), AttentionClassifier (src/models/text/attention_classifier.py) or
 * PretrainedAttentionClassifier (attention_classifier.py:74-132: frozen embedding tables, see mile_set_embedding).
 * ATTN_WIDE is the AttentionClassifier again, on the kernel that streams its weights (emb_size <= 192, qkv_dim <= 128,
 * projections <= 128: the reference's pretraining shapes); ATTN keeps the on-chip kernel and its limits. */
typedef enum mile_model {
  MILE_MODEL_FCN = 0, MILE_MODEL_LENET = 1, MILE_MODEL_LENETTI = 2, MILE_MODEL_ATTN = 3, MILE_MODEL_ATTN_PRETRAINED = 4,
  MILE_MODEL_ATTN_WIDE = 5
} mile_model;

/* FCNConfig (src/config/models/fcn.py:7-30) + PriorConfig (src/config/sampler.py:60-95)
 * + Task: everything log_unnormalized_posterior (src/training/probabilistic.py:115-138)
 * closes over, apart from the data. */
typedef struct mile_model_spec {
  int32_t in_features;               /* F: columns of X */
  int32_t n_layers;                  /* len(hidden_structure); last entry is the output layer */
  int32_t widths[MILE_MAX_LAYERS];   /* hidden_structure */
  int32_t activation;                /* mile_activation, between layers, none after the last */
  int32_t task;                      /* mile_task: regr -> output width 2 (mu, log sigma) */
  int32_t prior;                     /* mile_prior */
  float prior_loc;
  float prior_scale;
  int32_t use_bias;                  /* FCNConfig.use_bias; only 1 is supported (ATTN: AttentionClassifierConfig.bias, 0 or 1) */
  int32_t model;                     /* mile_model.  LENET: X rows are NCHW images, in_features = C*H*W,
                                      * n_layers = 1 and widths[0] = out_dim; parameter order is ravel_pytree's
                                      * (conv1, conv2, fc1, fc2, fc3; bias before kernel [kh,kw,in,out]).
                                      * LENETTI: the same conventions; parameters conv1 (3x3, 1 output channel), fc1
                                      * ((H+2)(W+2) -> 8), fc2, fc3 (8 -> 8), fc4 (8 -> out_dim).
                                      * ATTN: X rows are T token ids stored as fp32 (exact below 2^24; the host checks
                                      * 0 <= id < vocab_size, 0 is the pad id), in_features = ctx_len = T, task
                                      * classification, widths = projection_dim + [n_classes] (n_layers = 1..3).
                                      * Parameters in ravel_pytree order (sorted keys, bias before kernel; biases only
                                      * with use_bias): MDPA.key [C,H,hd], MDPA.out [H,hd,C], MDPA.query, MDPA.value,
                                      * TokenEmbedding_0.Embedding.embedding [V,C], .PositionEmbedding.embedding [T,C],
                                      * classifier [P_last,K], projection_0 [C,P_0], projection_1 [P_0,P_1].
                                      * ATTN_PRETRAINED: the same geometry fields and conventions; one more gelu before
                                      * the classifier; no TokenEmbedding_0 leaves (the tables are not parameters: they
                                      * come from mile_set_embedding).
                                      * ATTN_WIDE: ATTN's model, parameters and conventions exactly; only the limits
                                      * differ (those of ATTN_PRETRAINED) */
  int32_t img_c;                     /* LENET / LENETTI image geometry (ignored for the FCN) */
  int32_t img_h;
  int32_t img_w;
  int32_t vocab_size;                /* ATTN geometry (ignored otherwise): V */
  int32_t ctx_len;                   /* T (== in_features) */
  int32_t emb_size;                  /* C */
  int32_t n_heads;                   /* H */
  int32_t qkv_dim;                   /* D; H divides D, head size hd = D / H */
} mile_model_spec;

/* blackjax IntegratorState(position, momentum, logdensity, logdensity_grad) for an
 * ensemble (src/types.py:17-27 State is its `position` prefix). */
typedef struct mile_state {
  int32_t n_particles;       /* E */
  float *position;           /* [E, d] */
  float *momentum;           /* [E, d], unit rows */
  float *logdensity;         /* [E] */
  float *logdensity_grad;    /* [E, d] */
} mile_state;

/* Arguments of n_steps kernel steps == the lax.scan body of
 * src/training/sampling.py:140-178 run n_steps times. */
typedef struct mile_step_args {
  const float *step_size;        /* [E] per-chain step size (warmup_params.txt line 1) */
  const float *L;                /* [E] per-chain momentum decoherence length (line 2) */
  const float *sqrt_diag_cov;    /* [E, d] or NULL (== 1.0, what blackjax.mclmc defaults to) */
  const float *noise;            /* [n_steps, 2, E, d] N(0,1) draws (parity mode) or NULL */
  uint64_t seed;                 /* counter RNG (Philox4x32-10 + Box-Muller) when noise == NULL */
  const int32_t *particle_ids;   /* [E] GLOBAL chain ids keying the RNG streams, or NULL => 0..E-1 */
  int64_t step_offset;           /* index of the first step: RNG counter and thinning predicate */
  int32_t n_steps;
  int32_t n_thinning;            /* keep position when (step_offset+i) % n_thinning == 0; <=0: keep none */
  int32_t refresh;               /* mile_refresh */
  float *out_samples;            /* [n_kept, E, d] kept positions in step order, or NULL */
  float *out_info;               /* [n_steps, E, 3] (logdensity, kinetic_change, energy_change) or NULL */
} mile_step_args;

/* Arguments of n_steps warm-up steps with on-device step-size adaptation == the scan body `step`
 * of make_L_step_size_adaptation (src/training/warmup.py:271-363): kernel step, handle_nans
 * (:468-483), the energy-variance step-size predictor, and the streaming averages of x and x^2
 * that give L = sqrt(sum Var[x_i]) after tune2.  One tuner per chain; all arrays are device
 * memory owned by the caller and updated in place. */
typedef struct mile_tune_args {
  float *step_size;              /* [E] in/out */
  const float *L;                /* [E] */
  const float *sqrt_diag_cov;    /* [E, d] or NULL */
  float *step_size_max;          /* [E] in/out, start at +inf */
  float *time;                   /* [E] in/out, start at 0 */
  float *x_average;              /* [E] in/out, start at 0 */
  float *stream_weight;          /* [E] in/out, start at 0 */
  float *stream_average;         /* [E, 2, d] in/out, start at 0: weighted means of x and x^2 */
  const float *noise;            /* [n_steps, 2, E, d] or NULL (counter RNG) */
  uint64_t seed;
  const int32_t *particle_ids;   /* [E] or NULL */
  int64_t step_offset;           /* RNG step counter of the first step */
  int32_t n_steps;
  int32_t schedule_step0;        /* position of the first step in the schedule (0 .. tune1+tune2) */
  int32_t n_mask_steps;          /* schedule positions < n_mask_steps are tune1 (mask = 1: no averaging) */
  int32_t schedule_total;        /* tune1 + tune2 + 1 (warmup.py:251,259) */
  float desired_energy_var_start;
  float desired_energy_var_end;  /* linear decay, or exponential with tau = total/4 when start > 2 */
  float trust_in_estimate;
  float decay_rate;              /* (n_eff - 1) / (n_eff + 1) */
  int32_t refresh;               /* mile_refresh */
  float *out_info;               /* [n_steps, E, 3] or NULL */
} mile_tune_args;

/* Optimizer of the warm-start stage (src/config/warmstart.py: OptimizerConfig -> optax; src/training/trainer.py:390-538). */
typedef enum mile_optimizer { MILE_OPT_SGD = 0, MILE_OPT_ADAM = 1, MILE_OPT_ADAMW = 2 } mile_optimizer;

/* One optimizer step of the deep-ensemble members on the current row window (round 3).  Update rules as optax writes them:
 * m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2, bias-corrected with step count t, update = lr (m^ / (sqrt(v^) + eps)
 * [+ weight_decay theta for adamw]); sgd: lr g.  g is the gradient of the batch-MEAN negative log-likelihood (no prior:
 * src/training/trainer.py:729-737). */
typedef struct mile_optim_args {
  int32_t kind;                  /* mile_optimizer */
  float learning_rate, b1, b2, eps, weight_decay;
  int64_t t;                     /* step count including this step (bias correction) */
  float *m, *v;                  /* [E, d] moments, caller-owned, updated in place (unused for sgd: may be NULL) */
  const uint8_t *active;         /* [E] 1 = still training; 0 = early-stopped: parameters AND moments stay frozen.  NULL = all */
  float *out_nll;                /* [E] batch-mean negative log-likelihood at the parameters BEFORE the update, or NULL */
} mile_optim_args;

/* Arguments of n_steps NUTS steps == blackjax.nuts(logdensity_fn, step_size, inverse_mass_matrix, max_num_doublings,
 * divergence_threshold).step (blackjax 1.2.2 nuts.build_kernel with integrators.velocity_verlet and
 * metrics.default_metric of a diagonal inverse mass matrix) run n_steps times (src/training/sampling.py:140-178 with
 * sampler.name 'nuts').  All chains build their trees in lockstep: one grad launch per leapfrog round.
 * Random draws of step i (global step index step_offset + i): momentum normals, Philox stage 3 (same quad layout as the
 * MCLMC noise); uniforms, Philox stage 4, counter word 0 = slot with M = max_num_doublings:
 *   slot j in [0, M): direction of doubling j (forward when u < 0.5); slot M + j: progressive_biased_sampling of doubling j;
 *   slot 2M + n: progressive_uniform_sampling of the n-th leapfrog leaf of the step (n = 0, 1, ...; the first leaf of a
 *   subtree draws none).  Explicit draws use the same slots. */
typedef struct mile_nuts_args {
  const float *step_size;            /* [E] (ignored by mile_nuts_warmup: the adaptation state's) */
  const float *inverse_mass_matrix;  /* [E, d] diagonal (ignored by mile_nuts_warmup) */
  int32_t max_num_doublings;         /* 1..12, <= the value given to mile_nuts_reserve; blackjax default 10 */
  float divergence_threshold;        /* blackjax default 1000: a leaf with energy - initial energy above it diverges */
  const float *momentum_noise;       /* [n_steps, E, d] N(0,1) draws (parity mode) or NULL */
  const float *uniforms;             /* [n_steps, E, 2 M + 2^M] U(0,1) draws by slot (parity mode) or NULL */
  uint64_t seed;                     /* counter RNG when the explicit draws are NULL */
  const int32_t *particle_ids;       /* [E] GLOBAL chain ids keying the RNG streams, or NULL => 0..E-1 */
  int64_t step_offset;               /* index of the first step: RNG counter and thinning predicate */
  int32_t n_steps;
  int32_t n_thinning;                /* keep position when (step_offset+i) % n_thinning == 0; <=0: keep none */
  float *out_samples;                /* [n_kept, E, d] kept positions in step order, or NULL */
  float *out_info;                   /* [n_steps, E, 6] NUTSInfo (num_integration_steps, acceptance_rate,
                                        num_trajectory_expansions, is_divergent, energy, is_turning) or NULL */
  int64_t *out_stats;                /* HOST [2] or NULL: leapfrog rounds launched and host syncs, ADDED to */
} mile_nuts_args;

/* Window adaptation state (blackjax 1.2.2 adaptation.window_adaptation.base with a diagonal mass matrix), one per chain,
 * caller-owned device memory updated in place by mile_nuts_warmup.  Start: step_size = initial_step_size,
 * inverse_mass_matrix = 1, da = (log eps0, 0, 1, 0, log(10 eps0)), welford = 0, welford_count = 0.  After the last
 * warm-up step the tuned step size is exp(da[:, 1]) (window_adaptation final). */
typedef struct mile_nuts_adapt_args {
  float *step_size;                  /* [E] in/out: exp(log_step_size), the step size of the next step */
  float *inverse_mass_matrix;        /* [E, d] in/out */
  float *da;                         /* [E, 5] in/out: log_step_size, log_step_size_avg, step, avg_error, mu */
  float *welford;                    /* [E, 2, d] in/out: mean, m2 of the positions in the current slow window */
  float *welford_count;              /* [E] in/out */
  const int32_t *schedule;           /* HOST [n_steps, 2]: (stage, is_middle_window_end) of build_schedule, from the
                                        caller's schedule position of the first step; stage 1 = slow window */
  float target_acceptance_rate;      /* 0.8 */
} mile_nuts_adapt_args;

typedef struct mile_sampler mile_sampler;

const char *mile_last_error(void);
int32_t mile_abi_version(void);

/* Replaces: config.kernel(logdensity_fn, ...) construction of the target, i.e.
 * ProbabilisticModel.__init__ (src/training/probabilistic.py:19-47) + Prior.from_name
 * (src/training/priors.py:67-91).  `device` is the HIP device ordinal. */
int32_t mile_create(const mile_model_spec *spec, int32_t device, mile_sampler **out);
int32_t mile_destroy(mile_sampler *s);

/* pytree_size(position) (blackjax.util; src/training/warmup.py:203). */
int64_t mile_param_count(const mile_sampler *s);

/* Offsets of layer `layer`'s bias and kernel inside the raveled vector (ravel_pytree order).  LENET: layers 0..4 = conv1, conv2,
 * fc1, fc2, fc3; LENETTI: layers 0..4 = conv1, fc1, fc2, fc3, fc4; ATTN and ATTN_WIDE: layers 0..3 = MDPA key, out, query, value,
 * 4 = Embedding (kernel = the table, no bias), 5 = PositionEmbedding, 6 = classifier, 7.. = projection_0, projection_1;
 * ATTN_PRETRAINED: layers 0..3 = MDPA key, out, query, value, 4 = classifier, 5.. = projection_0, projection_1.
 * A missing bias (use_bias = 0) has offset -1. */
int32_t mile_param_offsets(const mile_sampler *s, int32_t layer, int64_t *bias_off, int64_t *kernel_off);

/* Replaces: partial(log_unnormalized_posterior, x=train_x, y=train_y)
 * (src/training/trainer.py:576-580).  X [N, F] fp32; y [N] fp32 (regr) or int32 (classification). */
int32_t mile_set_data(mile_sampler *s, const float *X, const void *y, int64_t N, void *stream);

/* MILE_MODEL_ATTN_PRETRAINED only: PretrainedTokenEmbedding (src/flax_building_blocks/basic.py:117-143).  Copies the frozen
 * token table emb [V, C] and the first T rows of the position table, pos [T, C], into buffers the sampler owns (shared by all
 * chains; they are neither sampled nor in the prior).  Until it has been called, mile_logpost_grad, mile_warmstart_step,
 * mile_init, mile_step, mile_tune, mile_nuts_step, mile_nuts_warmup, mile_pointwise_loglik and mile_predict fail with
 * MILE_ERR_STATE.
 * Calling it again replaces the tables. */
int32_t mile_set_embedding(mile_sampler *s, const float *emb, const float *pos, void *stream);

/* Restrict the likelihood to rows [begin, begin + count) of the training set for the following mile_logpost_grad calls
 * (count = 0: all rows again).  Replaces the minibatches of the warm-start stage: loader.iter(split='train', batch_size=...)
 * (src/dataset/tabular.py:170-212) feeding single_step_regr / single_step_class (src/training/trainer.py:706-760).
 * Supported by MILE_GRAD_GENERIC, the MFMA_NARROW, MFMA_W64, MFMA_WIDE, LENET, LENETTI and ATTN* kernels (mile_logpost_grad fails with MILE_ERR_STATE on
 * MFMA_W128_BF16 / GEMM_F32 under a window); the MCLMC path itself is full-batch (n_batches = 1). */
int32_t mile_set_row_window(mile_sampler *s, int64_t begin, int64_t count);

/* Replaces: one `single_step_regr` / `single_step_class` + `optimizer.update` + `optax.apply_updates` of the warm-start loop
 * (src/training/trainer.py:706-760, 430-470) for all E members at once: the likelihood gradient of the rows selected by
 * mile_set_row_window (the minibatch; all rows without a window) from the grad kernel, then ONE fused launch that forms the
 * batch-mean NLL gradient from the partial-gradient slabs, updates the moments and the parameters in place.  theta [E, d].
 * Grad kernels with row windows only (see mile_set_row_window). */
int32_t mile_warmstart_step(mile_sampler *s, float *theta, int32_t E, const mile_optim_args *args, void *stream);

/* Size the internal workspace (partial-gradient slabs etc.) for ensembles of up to E
 * particles.  Allocation happens here, never inside a launch call.  The slabs are [E, S, d] floats, S the row ranges of
 * the grad kernel.  ATTN_WIDE: a slab row holds the [V][C] table block, and S is min(CUs / E, rows / 8) with no cap at 64
 * -- at V = 10 000, C = 192 (d = 1 989 218) one chain on N >= 2048 rows reserves 256 rows = 2.04 GB, eight chains 8 x 32
 * rows = 2.04 GB as well (mile_slab_bytes reports it).  S is the largest row-range count among the kernels that run the model. */
int32_t mile_reserve(mile_sampler *s, int32_t E);

/* Bytes of the [E, S, d] partial-gradient slabs the workspace holds now (0 before the first mile_reserve). */
int64_t mile_slab_bytes(const mile_sampler *s);

/* Select the grad kernel (default AUTO). */
int32_t mile_set_grad_kernel(mile_sampler *s, int32_t which);
int32_t mile_get_grad_kernel(const mile_sampler *s);

/* Replaces: jax.value_and_grad(logdensity_fn)(position) as used inside blackjax
 * (integrators.py position update; mclmc.init).  theta [E, d] -> logp [E], grad [E, d]. */
int32_t mile_logpost_grad(mile_sampler *s, const float *theta, int32_t E, float *logp, float *grad,
                          void *stream);

/* Replaces: blackjax.mcmc.mclmc.init(position, logdensity_fn, rng_key)
 * (src/training/warmup.py:539-541).  Fills state->momentum = z/|z| with z = `noise` [E, d] if
 * non-NULL, else Philox(seed, particle id, step 0, stage 2); evaluates logdensity and its
 * gradient at state->position (which the caller has filled). */
int32_t mile_init(mile_sampler *s, mile_state *state, const float *noise, uint64_t seed,
                  const int32_t *particle_ids, void *stream);

/* Replaces: the scan of sampler.step(rng_key, state) at src/training/sampling.py:140-178
 * (blackjax.mclmc(...).step == build_kernel(...)(rng_key, state, L, step_size),
 * src/training/warmup.py:286-291,427-432).  Advances `state` in place by n_steps. */
int32_t mile_step(mile_sampler *s, mile_state *state, const mile_step_args *args, void *stream);

/* Replaces: the lax.scan over `step` in make_L_step_size_adaptation.run_steps
 * (src/training/warmup.py:352-363), i.e. phases 1+2 of mclmc_find_L_and_step_size, on the device.
 * Advances `state` in place.  d <= 16384: the tuner runs inside the record-point update kernel; beyond that each
 * step is an ordinary kernel step followed by one tuner launch (k_tune_post), same arithmetic. */
int32_t mile_tune(mile_sampler *s, mile_state *state, const mile_tune_args *args, void *stream);

/* Replaces: the per-sample forward pass + log_prob of the evaluation path, i.e. predict_from_samples /
 * pointwise_lppd (src/inference/evaluation.py:16-43, src/inference/metrics.py:247-294).
 * theta [S, d] (S posterior samples, any chains), X [N, F] and y [N] (fp32 or int32 labels) are device
 * pointers of a TEST set (independent of mile_set_data); out [S, N] = log p(y_n | x_n, theta_s). */
int32_t mile_pointwise_loglik(mile_sampler *s, const float *theta, int32_t S, const float *X, const void *y,
                              int64_t N, float *out, void *stream);

/* Replaces: the per-sample module.apply of predict_from_samples / predict_bde (src/inference/evaluation.py:16-43,
 * 334-406), the input of every metric but LPPD (ACC, RMSE, coverage, calibration error).
 * theta [S, d] (any S >= 1) and X [N, F] as for mile_pointwise_loglik; no labels.  out [S, N, O] fp32 row-major, O the
 * width of the last layer: the RAW outputs -- (mu, log sigma) unclipped, or the logits before any softmax; NaN / inf
 * pass through.  Runs the forward kernels of mile_pointwise_loglik with the row's outputs stored instead of their
 * log-probability.  (Added under ABI 10: a new symbol, no struct or existing entry changed.) */
int32_t mile_predict(mile_sampler *s, const float *theta, int32_t S, const float *X, int64_t N, float *out, void *stream);

/* Posterior-predictive moments: the Bayesian-model-average prediction of S draws on N rows, reduced over the draw axis on
 * the device (the reference reduces predict_bde's [S, N, O] outputs on the host, src/inference/evaluation.py:459-543).
 * theta [S, d] full-layout (partition mode included) and X [N, F] as for mile_predict.  out [N, W] fp32 row-major,
 * W = mile_predict_moments_width:
 *   regression, W = 3:          out[n] = (mean_s mu, Var_s mu with divisor S: epistemic, mean_s sigma^2: aleatoric),
 *                               sigma = clip(exp(log sigma), 1e-6, 1e6) as in mile_pointwise_loglik; columns 1 + 2 are the
 *                               variance of the equal-weight mixture of the S Normals
 *   K classes, W = K + 2:       out[n, 0:K] = mean_s softmax, out[n, K] = its entropy (nats), out[n, K+1] = that entropy
 *                               minus mean_s of each draw's entropy (mutual information, clamped at 0); p = 0 adds 0
 * A draw with a non-finite raw output on row n is left out of row n's statistics (per draw and per row; the reference
 * drops whole chains); dropped [N] int32 (device, may be null) receives how many were.  A row with every draw left out
 * holds NaN.  The forward is mile_predict's, in passes of at most max_draws_per_pass draws (0: as many as fit 256 MiB of
 * raw outputs) into a workspace the handle owns and grows here -- never [S, N, O] at once; accumulators are fp64
 * (Welford + Chan for the variance), so the result does not depend on max_draws_per_pass beyond fp64 rounding.
 * MILE_ERR_INVALID: a null handle / theta / X / out, S < 1 or > 2^31 - 1, N < 1 or > 2^30 - 1, max_draws_per_pass < 0;
 * MILE_ERR_STATE: frozen tables not set; MILE_ERR_NOMEM: the workspace.  Nothing is launched on any of them.
 * The workspace is ONE buffer of the handle that mile_predict_moments, mile_predict_quantiles, mile_lppd_stream,
 * mile_loo_stream and mile_calibration_stream share: it is
 * as large as the largest of their calls so far asked for, each call lays its own blocks out in it, and -- like the staged
 * evaluation rows, which every evaluation call of a handle has always shared -- it holds one call at a time: evaluation calls
 * on one handle go on one stream, or are ordered by the caller.
 * (Added under ABI 10: two new symbols, no struct or existing entry changed.) */
int32_t mile_predict_moments(mile_sampler *s, const float *theta, int64_t S, const void *X, int64_t N, float *out,
                             int32_t *dropped, int64_t max_draws_per_pass, void *stream);
int32_t mile_predict_moments_width(const mile_sampler *s);

/* Exact predictive quantiles and probability integral transform of the ensemble.  On row n the predictive is the equal-weight
 * mixture of the kept draws' Normals, F_n(t) = mean_s Phi((t - mu_sn) / sigma_sn), sigma = clip(exp(log sigma), 1e-6, 1e6) as in
 * mile_pointwise_loglik; quant[n, i] is the root of F_n(t) = levels[i] and pit[n] = F_n(y_n).  y_n lies in the central
 * interval of coverage c exactly when |pit[n] - 1/2| <= c / 2.
 * raw [S, N, 2] fp32 (mu, log sigma) as mile_predict writes them; levels [Q] fp64 on the HOST, strictly inside (0, 1),
 * strictly increasing, 1 <= Q <= 32; y [N] fp32 device or null; quant [N, Q] fp32 or null; pit [N] fp32 or null (needs y);
 * dropped [N] int32 or null.
 * A draw is left out of row n if either of its two raw outputs there is NaN or +-inf (per draw and per row, the rule of
 * mile_predict_moments); dropped[n] counts them, and a row with nothing kept holds NaN in quant and pit.  Quantiles of
 * increasing levels are non-decreasing.  The root is bracketed exactly by min_s and max_s of mu_s + Phi^-1(p) sigma_s and
 * found by a bracketed Newton iteration on fp64 sums of Phi (through erfc) and of the density, all levels in one sweep over the
 * row's components, until the bracket is below 2^-25 max(|mid|, sd_n), sd_n the mixture's standard deviation; sums in a
 * fixed order, no atomics: a row's result depends on its S pairs alone, bit for bit.
 * mile_mixture_quantiles needs no handle (outputs from anywhere, a deep ensemble's members for example); its workspace (the
 * packed copy of a row tile, at most 256 MiB) is allocated and freed in the call, which returns after the kernels finish.
 * mile_predict_quantiles is the same for draws theta [S, d] full-layout on X [N, F]: mile_predict's forward, never
 * [S, N, 2] at once.  The rows go in tiles of Nt rows, [S][Nt][2] floats plus the packed copy within 256 MiB (Nt a multiple
 * of 32 where it can be; max_rows_per_tile > 0 caps it, 0: the library's choice); inside a tile the forward runs in passes of
 * at most max_draws_per_pass draws (0: all), each written at its draw offset, every (draw, row) forward exactly once.  The
 * workspace is the handle's and grown in the call; mile_predict_quantiles_workspace gives its bytes for (S, N) with the
 * library's tile, -1 for a null handle or a shape out of range.  The result is bitwise the same for every
 * max_draws_per_pass and max_rows_per_tile, and equal to mile_mixture_quantiles of mile_predict's outputs.
 * MILE_ERR_INVALID: a null raw / handle / theta / X / levels, S < 1 or > 2^31 - 1, N < 1 or > 2^30 - 1, Q outside [1, 32],
 * levels not strictly increasing or not strictly inside (0, 1), pit without y, neither quant nor pit, a negative pass or tile
 * size, a handle whose task is not regression; MILE_ERR_STATE: frozen tables not set; MILE_ERR_NOMEM: the workspace.
 * Nothing is launched on any of them.
 * (Added under ABI 10: three new symbols, no struct or existing entry changed.) */
int32_t mile_mixture_quantiles(const float *raw, int64_t S, int64_t N, const double *levels, int32_t Q, const float *y,
                               float *quant, float *pit, int32_t *dropped, void *stream);
int32_t mile_predict_quantiles(mile_sampler *s, const float *theta, int64_t S, const void *X, int64_t N,
                               const double *levels, int32_t Q, const float *y, float *quant, float *pit, int32_t *dropped,
                               int64_t max_draws_per_pass, int64_t max_rows_per_tile, void *stream);
int64_t mile_predict_quantiles_workspace(const mile_sampler *s, int64_t S, int64_t N);   /* bytes; -1 out of range */
/* The same for the chain-weighted mixture, the predictive that stacking weights describe; the conventions are those of
 * mile_mixture_crps.  raw [C * S, N, 2] fp32 (mu, log sigma), draw j of chain c at row c * S + j; weights [C] fp64 on the HOST,
 * every entry finite and >= 0, |sum_c w_c - 1| <= 1e-9.  On row n a draw with a non-finite mu or log sigma is left out of that
 * row, K_c counts chain c's kept draws and dropped[c][n] = S - K_c (dropped [C, N] int32 or null); sigma = clip(exp(log sigma),
 * 1e-6, 1e6), formed in fp64 where it is used.  The weighted CDF is
 *   F_n(t) = sum_c (w_c / K_c) sum_{i in c, kept} Phi((t - mu_i) / sigma_i),
 * quant[n, q] is the root of F_n(t) = levels[q] and pit[n] = F_n(y_n).  A chain with w_c = 0 enters no sum, so its non-finite
 * draws cannot poison a row; a chain with w_c > 0 and K_c = 0 makes the row NaN in quant and pit.  Quantiles of increasing
 * levels are non-decreasing.  The bracket of the unweighted solver stays exact for any convex combination: min and max of
 * mu_i + Phi^-1(p) sigma_i over the components that carry weight; the iteration is the unweighted one, with w_c / K_c
 * multiplied into Phi and the density, and stops at a bracket below 2^-25 max(|mid|, sd_n), sd_n the weighted mixture's
 * standard deviation.  fp64 sums in a fixed order, no floating-point atomics: a row's result depends on its C * S pairs and
 * the weights alone, bit for bit.  With w_c = 1 / C and nothing dropped it is the predictive of mile_mixture_quantiles (equal
 * within the solver's tolerance, not bitwise: the sums differ in their last bits).
 * mile_predict_quantiles_weighted is the same for draws theta [C * S, d] on X [N, F], with the tiles, passes and shared
 * workspace of mile_predict_quantiles (mile_predict_quantiles_weighted_workspace: its bytes); the result is bitwise the same
 * for every max_draws_per_pass and max_rows_per_tile, and equal to mile_mixture_quantiles_weighted of mile_predict's outputs.
 * It records no sweeps for mile_debug_quantile_sweeps.
 * MILE_ERR_INVALID, nothing launched: the refusals of the unweighted pair (with C * S for S), C < 1 or > 1024,
 * C * S > 2^31 - 1, null weights, a negative or non-finite weight, a weight sum off by more than 1e-9.
 * (Added under ABI 10: three new symbols, no struct or existing entry changed.) */
int32_t mile_mixture_quantiles_weighted(const float *raw, int32_t C, int64_t S, int64_t N, const double *weights,
                                        const double *levels, int32_t Q, const float *y, float *quant, float *pit,
                                        int32_t *dropped /* [C, N] */, void *stream);
int32_t mile_predict_quantiles_weighted(mile_sampler *s, const float *theta /* [C*S, d] */, int32_t C, int64_t S, const void *X,
                                        int64_t N, const double *weights, const double *levels, int32_t Q, const float *y,
                                        float *quant, float *pit, int32_t *dropped, int64_t max_draws_per_pass,
                                        int64_t max_rows_per_tile, void *stream);
int64_t mile_predict_quantiles_weighted_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N);   /* bytes; -1 out of range */
/* Test and tool hook: over the rows of the handle's last mile_predict_quantiles that asked for quantiles, the row count, the
 * sum of the solver's sweeps and the largest sweep count of a row (synchronises the device).  The sweep counts lie in the
 * shared evaluation workspace: once a later mile_predict_moments, mile_lppd_stream, mile_loo_stream, mile_calibration_stream or
 * mile_predict_quantiles has reserved it they are gone, and this reports 0 rows (never stale counts) until a mile_predict_quantiles has finished again. */
int32_t mile_debug_quantile_sweeps(mile_sampler *s, int64_t *rows, int64_t *total, int32_t *most);

/* PSIS-LOO and WAIC of the ensemble on the rows the sampler conditioned on: Pareto-smoothed importance-sampling leave-one-out
 * cross-validation (Vehtari, Gelman & Gabry 2017; Vehtari et al. 2024; the generalised-Pareto fit of Zhang & Stephens 2009),
 * per row, on the device.  The reference has no counterpart.  For row n let l_s = log p(y_n | x_n, theta_s) over all S draws
 * pooled over chains (fp32 as mile_pointwise_loglik writes them; all arithmetic below is fp64).
 *   A draw whose l_s is NaN or +-inf is left out of row n (per draw and per row, the rule of mile_predict_moments);
 *   dropped[n] counts them, S_n are kept, and a row with S_n < 2 holds NaN in every other output.
 *   lppd[n]   = logsumexp_s l_s - log S_n
 *   p_waic[n] = sum_s (l_s - mean l)^2 / (S_n - 1)  (Welford per thread, Chan's merge in a fixed order); elpd_waic = lppd - p_waic
 *   r_s = -l_s - max_s(-l_s); M = ceil(fmin(S_n / 5.0, 3.0 * sqrt(S_n / r_eff))); the tail is the M largest r_s (ties at the
 *   boundary broken in any way: every output is a sum that cannot see the choice); cut = max((M+1)-th largest r, log DBL_MIN),
 *   ec = exp(cut), x_i = exp(r_(i)) - ec for the tail in ascending order, i = 1 .. M.
 *   The fit runs if M >= 5 and x_q > 0, q = floor(M / 4 + 0.5): m = 30 + floor(sqrt(M)); for j = 1 .. m
 *   b_j = (1 - sqrt(m / (j - 0.5))) / (3 x_q) + 1 / x_M, k_j = mean_i log1p(-b_j x_i), L_j = M (log(-b_j / k_j) - k_j - 1),
 *   w_j = 1 / sum_i exp(L_i - L_j) (a sum that overflows gives weight 0); b = sum_j b_j w_j, k = mean_i log1p(-b x_i),
 *   sigma = -k / b, khat = (M k + 5) / (M + 10).  Without a fit, or with a non-finite khat or sigma, khat[n] = NaN and
 *   nothing is smoothed.  With one, tail rank i takes lw = log(sigma expm1(-khat log1p(-p_i)) / khat + ec),
 *   p_i = (i - 0.5) / M (at khat == 0: -sigma log1p(-p_i) in place of the quotient); every other draw keeps lw = r_s; then
 *   lw = min(lw, 0), lw -= logsumexp_s lw, and elpd_loo[n] = logsumexp_s(lw_s + l_s).
 * lppd, p_waic, elpd_loo, khat [N] fp64 and dropped [N] int32 are device pointers; each may be null, but not all five.
 * r_eff, the relative efficiency of the draws, is a finite positive host scalar (1: independent draws).
 * mile_psis_loo needs no handle: loglik [S, N] from anywhere; its workspace (the packed copy of a row tile, at most 256 MiB)
 * is allocated and freed in the call, which returns after the kernels finish.
 * mile_loo_stream is the same for draws theta [S, d] full-layout on (X [N, F], y [N]) as for mile_pointwise_loglik, whose
 * forward it runs, never [S, N] at once.  The rows go in tiles of Nt rows, [S][Nt] floats plus the packed [Nt][S] copy within
 * 256 MiB (Nt a multiple of 32 where it can be; max_rows_per_tile > 0 caps it, 0: the library's choice); inside a tile the
 * forward runs in passes of at most max_draws_per_pass draws (0: all), each written at its draw offset, every (draw, row)
 * forward exactly once.  The workspace is the handle's shared one, grown in the call; mile_loo_stream_workspace gives its
 * bytes for (S, N) with the library's tile, -1 for a null handle or a shape out of range.
 * Sums run in a fixed order without floating-point atomics and a row's result depends on its S values alone: the outputs
 * are bitwise the same for every max_draws_per_pass and max_rows_per_tile, and equal to mile_psis_loo of
 * mile_pointwise_loglik's tensor.
 * MILE_ERR_INVALID: a null loglik / handle / theta / X / y, no output asked for, S < 2 or > 2^20, N < 1 or > 2^30 - 1,
 * r_eff not finite or <= 0, a tail of more than 4096 draws (M at S_n = S; M <= 3072 whenever r_eff >= 1), a negative pass or
 * tile size; MILE_ERR_STATE: frozen tables not set; MILE_ERR_NOMEM: the workspace.  Nothing is launched on any of them.
 * (Added under ABI 10: three new symbols, no struct or existing entry changed.) */
int32_t mile_psis_loo(const float *loglik, int64_t S, int64_t N, double r_eff, double *lppd, double *p_waic, double *elpd_loo,
                      double *khat, int32_t *dropped, void *stream);
int32_t mile_loo_stream(mile_sampler *s, const float *theta, int64_t S, const void *X, const void *y, int64_t N, double r_eff,
                        double *lppd, double *p_waic, double *elpd_loo, double *khat, int32_t *dropped, int64_t max_draws_per_pass,
                        int64_t max_rows_per_tile, void *stream);
int64_t mile_loo_stream_workspace(const mile_sampler *s, int64_t S, int64_t N);   /* bytes; -1 out of range */

/* PSIS-LOO and WAIC of every chain on its own: mile_loo_stream for theta [C * S, d] full-layout, draw j of chain c at row
 * c * S + j as for mile_lppd_stream.  lppd, p_waic, elpd_loo, khat [C, N] fp64 and dropped [C, N] int32 are device pointers;
 * each may be null, but not all five.  A row tile is staged once for all chains; each chain's S draws then go through the tile
 * and pass scheme and the two kernels of mile_loo_stream, every (draw, row) forward exactly once, so row c of every output is
 * bitwise what mile_loo_stream gives for theta + c * S * d alone, for every max_draws_per_pass and max_rows_per_tile.  A call
 * that asks for lppd alone ends each row after its first pass: the [C, N] matrix of a held-out split.  The workspace is the
 * handle's shared one and that of one chain (mile_chain_loo_stream_workspace).
 * Limits and refusals are mile_loo_stream's, S being the draws of one chain, plus MILE_ERR_INVALID for C < 1 or > 1024.
 * (Added under ABI 10: two new symbols, no struct or existing entry changed.) */
int32_t mile_chain_loo_stream(mile_sampler *s, const float *theta, int32_t C, int64_t S, const void *X, const void *y, int64_t N,
                              double r_eff, double *lppd, double *p_waic, double *elpd_loo, double *khat, int32_t *dropped,
                              int64_t max_draws_per_pass, int64_t max_rows_per_tile, void *stream);
int64_t mile_chain_loo_stream_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N);   /* bytes; -1 out of range */

/* PSIS-LOO expectations and LOO-PIT of the ensemble: the importance weights that mile_psis_loo forms and discards, kept per draw,
 * and with them the leave-one-out expectation of any per-draw quantity (E_loo and loo_pit of the loo package and of ArviZ), per
 * row, on the device.  The reference has no counterpart.  For row n, l_s, the kept draws, M, the cut, the fit and the smoothed and
 * capped log weights lw_s with their normalisation lw_s -= logsumexp_s lw are exactly those of mile_psis_loo above.  Then
 *   w_s = exp(lw_s) for a kept draw, 0 for a dropped one (whose values are never read into a sum).
 *   Tie rule: draws of a row whose fp32 l_s have equal bits share the mean of their weights -- ties inside the tail, where the
 *   smoothed weight goes by rank, and ties across the tail's boundary, where some copies are smoothed and some are not.  Every
 *   output is then a function of the multiset {(l_s, h(s))} and does not change under a permutation of the draws (up to the
 *   rounding of a sum in another order); sum_s w_s = 1 and elpd_loo = log sum_s w_s exp(l_s) are what they were.
 *   expect[n][q]    = sum_s w_s h_q(s, n)                for Q columns h_q of per-draw values
 *   posterior[n][q] = (1 / S_n) sum_{kept s} h_q(s, n)   the in-sample counterpart: the difference is the optimism
 *   ess_w[n]        = 1 / sum_s w_s^2
 *   khat[n], elpd_loo[n], dropped[n] as mile_psis_loo gives them.
 *   A non-finite value of a kept draw goes into the sums of its (row, column) by IEEE rules and into no other.  A row with
 *   S_n < 2 holds NaN in every fp64 output (its row of weights included).
 * mile_psis_expect needs no handle: loglik [S, N] fp32 and values [S, N, Q] fp32 from anywhere, 1 <= Q <= 64.  expect, posterior
 * [N, Q], ess_w, khat, elpd_loo [N] (fp64), dropped [N] int32 and weights [N, S] fp64 (row n: the S weights in draw order) are
 * device pointers; each may be null, but not all; values may be null if neither expect nor posterior is asked for.  The
 * workspace (a row tile's packed l, its weights where the caller takes none, the partial sums; within 256 MiB) is allocated and
 * freed in the call, which returns after the kernels finish.
 * mile_loo_predict_stream forms the columns itself, for draws theta [S, d] full-layout on (X [N, F], y [N]), from ONE forward
 * per (draw, row): mile_predict's outputs z of the row tile.  l_s = the likelihood head of mile_pointwise_loglik on those z (the
 * same fp32 operations: khat, elpd_loo and dropped are mile_loo_stream's).  The columns are formed in fp64 from the fp32 z:
 *   regression (mu, log sigma), Q = 4: mu, mu^2, sigma^2, Phi((y - mu) / sigma) = 0.5 erfc(-(y - mu) / (sigma sqrt 2)), with
 *   sigma = exp(log sigma) clipped to [1e-6, 1e6] -- so expect gives the LOO predictive mean, E[mu^2] (epistemic variance
 *   E[mu^2] - E[mu]^2), the aleatoric variance E[sigma^2] and the LOO-PIT of y_n;
 *   classification with K <= 64 classes, Q = K: softmax(z) -- the LOO class probabilities.
 * Rows go in tiles of Nt rows: per (draw, row) the forward's block 4 O bytes, the packed l 4 and the weight 8, plus the partial
 * sums per row, within 256 MiB (Nt a multiple of 32 where it can be; max_rows_per_tile > 0 caps it); inside a tile the forward
 * runs in passes of at most max_draws_per_pass draws (0: all).  The workspace is the handle's shared one;
 * mile_loo_predict_stream_workspace gives its bytes for (S, N) with the library's tile, -1 for a null handle, a shape out of
 * range or a head the call refuses.
 * The sums over draws run in fp64 over runs of the draw axis whose boundaries depend on S and Q alone, each run in index order,
 * the runs combined in index order, without floating-point atomics: a row's result depends on its own S draws alone, and the
 * outputs are bitwise the same for every max_draws_per_pass and max_rows_per_tile.
 * MILE_ERR_INVALID: the refusals of mile_psis_loo / mile_loo_stream (null pointers, no output asked for, S, N, r_eff, the tail,
 * the pass and tile sizes), Q < 1 or > 64, expect or posterior without values, a regression head other than (mu, log sigma),
 * more than 64 classes (the unsupported-spec refusal: form the columns and call mile_psis_expect); MILE_ERR_STATE: frozen tables
 * not set; MILE_ERR_NOMEM: the workspace.  Nothing is launched on any of them.
 * (Added under ABI 10: three new symbols, no struct or existing entry changed.) */
int32_t mile_psis_expect(const float *loglik, const float *values, int64_t S, int64_t N, int32_t Q, double r_eff, double *expect,
                         double *posterior, double *ess_w, double *khat, double *elpd_loo, int32_t *dropped, double *weights,
                         void *stream);
int32_t mile_loo_predict_stream(mile_sampler *s, const float *theta, int64_t S, const void *X, const void *y, int64_t N, double r_eff,
                                double *expect, double *posterior, double *ess_w, double *khat, double *elpd_loo, int32_t *dropped,
                                int64_t max_draws_per_pass, int64_t max_rows_per_tile, void *stream);
int64_t mile_loo_predict_stream_workspace(const mile_sampler *s, int64_t S, int64_t N);   /* bytes; -1 out of range */

/* Stacking of chains that do not mix (Yao, Vehtari, Simpson & Gelman 2018; Yao, Vehtari & Gelman 2022): one evaluation of the
 * log score of the weighted mixture of the chains' pointwise predictive densities, with its gradient in the weights and the
 * Gram matrix of the responsibilities (the negative Hessian), on the device.  The reference has no counterpart.  No handle.
 * lpd [C, N] fp64 (say the elpd_loo of mile_chain_loo_stream) and w [C] fp64 with entries >= 0 are device pointers.  All
 * arithmetic is fp64.
 *   Row n is used iff no lpd[c][n] is NaN or +inf and m_n = max_c lpd[c][n] > -inf; any other row is left out, holds NaN in
 *   row_score and enters no sum; used[0] counts the rest.
 *   e_cn = exp(lpd[c][n] - m_n); mix_n = sum_c w_c e_cn in chain order (one fma per chain); row_score[n] = m_n + log mix_n;
 *   R_cn = e_cn / mix_n.
 *   score[0] = (sum_n row_score[n]) / used;  grad[c] = (sum_n R_cn) / used;  hess[a][b] = (sum_n R_an R_bn) / used.
 *   A used row with mix_n == 0 makes score -inf; grad and hess are then unspecified.  used == 0 makes all three NaN.
 *   hess is exactly symmetric: the lower triangle is computed and mirrored.
 * Sums over rows take a fixed two-stage order: blocks of B rows, each entry one chain of fma over the block's rows in row
 * order, then the blocks in block order; B depends on C and N alone (the blocks' partial sums within 64 MiB, at most 1024
 * blocks, B a multiple of 32).  No floating-point atomics.  The rows go in tiles whose responsibilities [C + 2][Nt] fp64 stay
 * within 256 MiB (max_rows_per_tile > 0 caps Nt, 0: the library's choice); a block that a tile cuts is carried from its
 * partial sum, so the outputs are bitwise the same for every max_rows_per_tile.
 * score [1], row_score [N], grad [C], hess [C, C] fp64 and used [1] int64 are device pointers; each may be null, but not all
 * five.  A call without hess computes only what score, grad and used need; one for row_score alone sums nothing.
 * The workspace is allocated and freed in the call, which returns after the kernels finish.
 * MILE_ERR_INVALID: a null lpd or w, C < 1 or > 1024, N < 1 or > 2^30 - 1, a negative tile size, no output asked for;
 * MILE_ERR_NOMEM: the workspace.  Nothing is launched on any of them.
 * (Added under ABI 10: a new symbol, no struct or existing entry changed.) */
int32_t mile_stack_eval(const double *lpd, const double *w, int32_t C, int64_t N, double *score, double *row_score, double *grad,
                        double *hess, int64_t *used, int64_t max_rows_per_tile, void *stream);

/* Exact CRPS (continuous ranked probability score) of the predictive mixture, per chain and for chain-weighted mixtures, on the
 * device.  Regression only; the reference has no counterpart.  raw [C * S, N, 2] fp32 (mu, log sigma) as mile_predict writes
 * them, draw j of chain c at row c * S + j as in mile_lppd_stream; y [N] fp32 device; weights [n_w, C] fp64 on the HOST,
 * 0 <= n_w <= 8, every vector >= 0, finite and summing to 1 within 1e-9.  mile_mixture_crps needs no handle.
 *   sigma = clip(expf(log sigma), 1e-6, 1e6) as in mile_pointwise_loglik.  A draw with a non-finite mu or log sigma on row n is
 *   left out of row n (per draw and per row, the rule of mile_predict_moments); K_c counts chain c's kept draws on the row and
 *   dropped[c][n] = S - K_c.
 *   A(d, v) = E|N(d, v)| = d erf(d / sqrt(2v)) + sqrt(2v / pi) exp(-d^2 / (2v)) >= 0.
 *   a_c = (1 / K_c) sum_{i in c} A(y - mu_i, sigma_i^2), fp64.
 *   G_cc' = (1 / (K_c K_c')) sum_{i in c} sum_{j in c'} A(mu_i - mu_j, sigma_i^2 + sigma_j^2), i = j included: pair terms in
 *   fp32, summed in fp32 over fixed runs of at most 32 terms and in fp64 beyond, in a fixed order; pairs i < j of one chain
 *   are computed once and counted twice, chain blocks c > c' are mirrored from c < c'.
 *   crps_chain[c][n] = a_c - G_cc / 2, spread_chain[c][n] = G_cc / 2: chain c alone.
 *   crps_mix[m][n] = sum_c w_c a_c - w'Gw / 2, spread_mix[m][n] = w'Gw / 2.  Row m = 0 is always the pooled ensemble,
 *   w_c = K_c / sum K (the equal-weight mixture of all kept draws, the predictive of mile_mixture_quantiles); rows 1 .. n_w are
 *   the caller's weight vectors in order.  A chain of weight 0 enters no sum.
 *   gram[n][c][c'] = G_cc', exactly symmetric.  2 G_cc' - G_cc - G_c'c' >= 0 is the energy distance between two chains'
 *   predictives on the row.
 *   A chain with K_c = 0 has NaN in its own outputs and in its row and column of gram, is skipped by the pooled weights and
 *   makes a caller's mixture with w_c > 0 NaN on that row; a row with nothing kept holds NaN everywhere.
 * No floating-point atomics; how the pairs are split over workgroups depends on (C, S, N) alone, so a row's outputs depend on
 * its draws alone, bit for bit.  The rows go in tiles (max_rows_per_tile > 0 caps them, 0: the library's choice) that keep a
 * launch of the pair kernel within 2^37 pairs -- a single row at the least -- and the workspace within the evaluation budget.
 * crps_chain, spread_chain [C, N], crps_mix, spread_mix [1 + n_w, N], gram [N, C, C] fp64 and dropped [C, N] int32 are device
 * pointers; each may be null, but not all six.  A call for dropped alone launches no pair kernel.
 * mile_mixture_crps allocates and frees its workspace in the call and returns after the kernels finish.
 * mile_crps_stream is the same for draws theta [C * S, d] full-layout on X [N, F]: mile_predict's forward runs in row tiles and
 * passes of at most max_draws_per_pass draws (0: all) into the handle's shared evaluation workspace, every (draw, row) forward
 * exactly once, [C * S, N, 2] never held at once.  Its outputs are bitwise the same for every pass and tile size and equal to
 * mile_mixture_crps of mile_predict's outputs.  mile_crps_stream_workspace: the bytes for the library's own tile.
 * MILE_ERR_INVALID: a null raw / handle / theta / X / y, no output asked for, C < 1 or > 1024, S < 1, C * S > 2^20, N < 1 or
 * > 2^30 - 1, n_w outside [0, 8] or n_w > 0 without weights, a weight negative or non-finite, |sum_c w_c - 1| > 1e-9, a negative
 * pass or tile size, a handle whose task is not regression; MILE_ERR_STATE: frozen tables not set; MILE_ERR_NOMEM: the
 * workspace.  Nothing is launched on any of them.
 * (Added under ABI 10: three new symbols, no struct or existing entry changed.) */
int32_t mile_mixture_crps(const float *raw, int32_t C, int64_t S, int64_t N, const float *y, const double *weights, int32_t n_w,
                          double *crps_chain, double *spread_chain, double *crps_mix, double *spread_mix, double *gram,
                          int32_t *dropped, int64_t max_rows_per_tile, void *stream);
int32_t mile_crps_stream(mile_sampler *s, const float *theta, int32_t C, int64_t S, const void *X, const float *y, int64_t N,
                         const double *weights, int32_t n_w, double *crps_chain, double *spread_chain, double *crps_mix,
                         double *spread_mix, double *gram, int32_t *dropped, int64_t max_draws_per_pass, int64_t max_rows_per_tile,
                         void *stream);
int64_t mile_crps_stream_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N);   /* bytes; -1 out of range */

/* Prediction sets and calibration of the classification ensemble, per chain and for the ensemble of all chains, on the device.
 * The reference stops before this (src/inference/evaluation.py:463-464).  raw [C * S, N, K] fp32 logits as mile_predict
 * writes them: draw j of chain c is row c * S + j, as in mile_lppd_stream (a deep ensemble's members are valid input).
 * y [N] int32 device labels, or null.  coverages [Q] fp64 on the HOST, strictly inside (0, 1), strictly increasing.
 * The groups are g = 0 .. C - 1 (each chain) and g = C (the ensemble), G = C + 1.  All arithmetic below is fp64.
 *   A draw is kept on row n iff all K logits there are finite (per draw and per row, the rule of mile_predict_moments).
 *   Per kept draw e_k = exp((double)z_k - (double)max_k z), p_k = e_k / sum_k e_k, the sum in class order.
 *   P[c][n][k] = (sum of p_k over chain c's kept draws in draw order) / kept[c][n]; P[C][n][k] = (sum of the chains' sums in
 *   chain order) / (sum of the chains' counts).  A (g, n) with nothing kept holds NaN in probs, has kept 0, is left out of
 *   group g's totals and bins, and its ensemble outputs are order = 0 .. K - 1, set_size = 0, rank = 0.
 *   Per (g, n) the classes are ordered by P descending, ties to the lower class index.  cum_i is the sequential sum of P in
 *   that order; size_q is the smallest m with cum_m >= coverages[q], or K if none reaches it.
 *   rank is the 1-based position of y_n in the order; covered_q = rank <= size_q; conf = P_(1); correct = (rank == 1);
 *   bin = min(n_bins - 1, (int)floor(conf * n_bins)); brier = sum_k (P_k - [k == y_n])^2 in class order; nll = -log P_y.
 *   A label outside [0, K) leaves the row out of the totals and bins, gives rank 0, and is counted in `bad labels`.
 * Outputs, device pointers, each may be null but not all: probs [G, N, K] fp64; kept [G, N] int32; order [N, K], set_size
 * [N, Q] and rank [N] int32, of the ensemble; totals [G, 5 + 2 Q] fp64 = (rows counted, rows correct, sum brier, sum nll,
 * bad labels, covered_q .., sum size_q ..); bins [G, n_bins, 3] fp64 = (count, sum conf, sum correct).  rank, totals and bins
 * need y.
 * Sums over rows take a fixed two-stage order: blocks of B rows (B a function of N, G, Q and n_bins alone) summed in row
 * order, then the blocks in block order; no floating-point atomics; counts are exact.
 * mile_calibration needs no handle: logits from anywhere; its workspace (a row tile's sums and records and the blocks'
 * partial sums, at most 256 MiB) is allocated and freed in the call, which returns after the kernels finish.
 * mile_calibration_stream is the same for draws theta [C * S, d] full-layout (partition mode included) on X [N, F]:
 * mile_predict's forward, never [C, S, N, K] at once.  The rows go in tiles of Nt rows (a multiple of 64 where it can be;
 * max_rows_per_tile > 0 caps it, 0: the library's choice), inside a tile the forward runs in passes of at most
 * max_draws_per_pass draws of every chain (0: as many as fit 128 MiB of logits), every (draw, row) forward exactly once.  The
 * workspace is the handle's shared one, grown in the call; mile_calibration_stream_workspace gives an upper bound of its
 * bytes for (C, S, N) with the library's tile and pass (over Q and n_bins), -1 for a null handle, a shape out of range or a
 * handle that the call would refuse.  The outputs are bitwise the same for every max_draws_per_pass and max_rows_per_tile,
 * and equal to mile_calibration of mile_predict's tensor.
 * MILE_ERR_INVALID: a null raw / handle / theta / X / coverages, no output asked for, C outside [1, 65535], S < 1 (or
 * C * S > 2^31 - 1), N < 1 or > 2^30 - 1, K outside [2, 64], Q outside [1, 16], coverages not strictly increasing or not
 * strictly inside (0, 1), n_bins outside [1, 64], rank / totals / bins without y, a negative pass or tile size, a handle
 * whose task is not classification or whose output width is not K (the stream takes K from the handle);
 * MILE_ERR_STATE: frozen tables not set; MILE_ERR_NOMEM: the workspace.  Nothing is launched on any of them.
 * (Added under ABI 10: three new symbols, no struct or existing entry changed.) */
int32_t mile_calibration(const float *raw, int32_t C, int64_t S, int64_t N, int32_t K, const void *y, const double *coverages,
                         int32_t Q, int32_t n_bins, double *probs, int32_t *kept, int32_t *order, int32_t *set_size, int32_t *rank,
                         double *totals, double *bins, void *stream);
int32_t mile_calibration_stream(mile_sampler *s, const float *theta, int32_t C, int64_t S, const void *X, const void *y, int64_t N,
                                const double *coverages, int32_t Q, int32_t n_bins, double *probs, int32_t *kept, int32_t *order,
                                int32_t *set_size, int32_t *rank, double *totals, double *bins, int64_t max_draws_per_pass,
                                int64_t max_rows_per_tile, void *stream);
int64_t mile_calibration_stream_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N);   /* bytes; -1 out of range */

/* Streamed LPPD and its running curves (the reference's lppd and running_lppd, src/inference/metrics.py:297-312, 408-446, and
 * the per-chain LPPD of src/inference/evaluation.py:520-529), reduced on the device without a [C, S, N] tensor.
 * theta [C * S, d] full-layout (partition mode included, as for mile_pointwise_loglik): draw j of chain c is row c * S + j.
 * X [N, F] and y [N] as for mile_pointwise_loglik.  curve_points [K] int32, 1 <= k_1 < ... < k_K <= S: the draw counts per
 * chain at which the curves are taken (read back to the host for their check).  With l = log p(y_n | x_n, theta_{c,j}),
 * A_k[c][n] = logsumexp over the first k draws of chain c, cnt_k(c, n) the draws of those that are not NaN:
 *   run_chain [K]:   mean_c mean_n (A_k - log cnt_k) at k = k_i: running_lppd at k, without exp(l) underflowing
 *   run_ens   [K]:   mean_n (logsumexp_c A_k - log sum_c cnt_k): lppd of the first k draws of all chains
 *   chain_lppd [C], row_lppd [N], lppd [1]: after all S draws, mean_n (A_S - log cnt_S) of each chain, the ensemble term of
 *                    each row, and its mean over the rows (= the last run_ens when k_K = S)
 *   dropped [C] int64: (draw, row) pairs of chain c left out
 * All fp64, all device pointers; an output not wanted is null (K = 0: no curve).
 * A draw whose log-likelihood on row n is NaN is left out of (chain c, row n) and counted (per draw and per row, the rule of
 * mile_predict_moments); +inf and -inf take part as values, -inf adding 0.  A (chain, row) with every draw left out makes
 * that chain's figures NaN, run_chain with them; the ensemble figures skip that chain on that row.
 * The forward is mile_pointwise_loglik's, the same window of at most max_draws_per_pass draws of every chain at a time
 * (0: as many as fit 256 MiB of [C * J, N] floats; at most 65535) into a workspace the handle owns and grows here; a pass is
 * split at each curve point.  The state is a streaming log-sum-exp (max, scaled sum) in fp64 per (chain, row), the row
 * means are a per-wave sum followed by a one-workgroup sum, both in a fixed order and without atomics: the outputs are
 * bitwise the same for every max_draws_per_pass.  mile_lppd_stream_workspace: bytes of the state and partial sums for
 * (C, N), what the workspace holds beyond the pass's [C * J, N] floats; -1 for a null handle or a shape out of range.
 * MILE_ERR_INVALID: a null handle / theta / X / y, C outside [1, 65535], S < 1, N < 1 or > 2^30 - 1, K < 0 or > S, K = 0
 * with run_chain or run_ens, K > 0 with null curve_points or without a curve output, no output at all, curve points not
 * strictly increasing or outside [1, S], max_draws_per_pass < 0; MILE_ERR_STATE: frozen tables not set; MILE_ERR_NOMEM: the
 * workspace.  Nothing is launched on any of them.
 * (Added under ABI 10: two new symbols, no struct or existing entry changed.) */
int32_t mile_lppd_stream(mile_sampler *s, const float *theta, int32_t C, int32_t S, const void *X, const void *y, int64_t N,
                         const int32_t *curve_points, int32_t K, double *run_chain, double *run_ens, double *chain_lppd,
                         double *row_lppd, double *lppd, int64_t *dropped, int64_t max_draws_per_pass, void *stream);
int64_t mile_lppd_stream_workspace(const mile_sampler *s, int32_t C, int64_t N);

/* Which outputs mile_chain_diagnostics computes (`what`), and how it reads its input. */
#define MILE_DIAG_WCV 1u
#define MILE_DIAG_BCV 2u
#define MILE_DIAG_ESS 4u
#define MILE_DIAG_CRHAT 8u
#define MILE_DIAG_RHAT 16u
#define MILE_DIAG_POOLED_INPUT 32u /* samples already hold the pooled normal scores: ESS and RHAT only */
#define MILE_DIAG_S_MIN 4
#define MILE_DIAG_S_MAX 4096
#define MILE_DIAG_POOL_MAX 16384   /* C * S up to which the pooled ranking runs in the library */

/* Replaces: between_chain_var, within_chain_var, effective_sample_size, split_chain_r_hat and gelman_split_r_hat
 * (src/inference/metrics.py:226-244, 354-405, 449-523), all rank-normalised as the reference's defaults, for every
 * parameter at once.  Needs no model, so it takes no mile_sampler; it launches on the current device.
 * samples [C][S][d] fp32, d contiguous (device).  Outputs (device, null where not asked for): wcv, bcv, rhat [d];
 * ess, crhat [C][d].  ess[c][p] is the single-chain estimator of mile_amd/diagnostics.py on chain c of the scores ranked
 * over all C*S draws of p; crhat[c][p] ranks chain c alone and splits it n_splits ways; rhat[p] uses all C*n_splits
 * pieces of the pooled scores.  Ties get their average rank; a NaN draw makes every score ranked with it NaN.
 * MILE_ERR_INVALID, with nothing launched: C outside [1, 65535], S outside [MILE_DIAG_S_MIN, MILE_DIAG_S_MAX], d < 1,
 * n_splits < 1 or not a divisor of S, S / n_splits < 2, no or unknown bits in `what`, a null pointer for an output asked
 * for, WCV / BCV / CRHAT together with MILE_DIAG_POOLED_INPUT, and ESS / RHAT on raw draws with C*S > MILE_DIAG_POOL_MAX
 * (rank those outside and pass the scores with MILE_DIAG_POOLED_INPUT).  MILE_ERR_STATE, with nothing launched: a workspace
 * below that of min(d, 32) parameters.  mile_chain_diagnostics_workspace returns the size that lets the call run in the
 * fewest launches it will use (parameters are walked in chunks that fit the workspace given); -1 for a bad shape.
 * (Added under ABI 10: two new symbols, no struct or existing entry changed.) */
int32_t mile_chain_diagnostics(const float *samples, int32_t C, int32_t S, int64_t d, int32_t n_splits, uint32_t what,
                               float *wcv, float *bcv, float *ess, float *crhat, float *rhat, void *workspace,
                               int64_t workspace_bytes, void *stream);
int64_t mile_chain_diagnostics_workspace(int32_t C, int32_t S, int64_t d, uint32_t what);

/* How mile_canonicalize_fcn orders the hidden units (`how`): one key, and optionally the sign fix. */
#define MILE_CANON_KEY_BIAS 0u
#define MILE_CANON_KEY_NORM 1u
#define MILE_CANON_SIGN     2u
#define MILE_CANON_WIDTH_MAX 1024

/* Canonical hidden-unit ordering of FCN draws: every draw is replaced by one representative of its orbit under the
 * permutations of the hidden units of each layer (and, with MILE_CANON_SIGN on a tanh net, their sign flips), so that
 * per-parameter statistics (mile_chain_diagnostics, trace and histogram plots, posterior summaries) of chains that sit in
 * permuted copies of one mode agree.  Needs no mile_sampler; launches on the current device.
 * theta [M][d] fp32 (device) holds draws of the MILE_MODEL_FCN `spec` in the library's full layout (mile_param_offsets).
 * Hidden layers are l = 0 .. n_layers - 2 with widths W_l; the output layer and the inputs never move.  H = sum_l W_l
 * (mile_canonical_hidden); hidden layer l owns [o_l, o_l + W_l) of the H axis.
 *   sign  (MILE_CANON_SIGN, MILE_ACT_TANH only) s_l[j] = -1 iff bias_l[j] < 0, else +1: -0.0, +0.0 and NaN are not flipped.
 *   key   MILE_CANON_KEY_BIAS: s_l[j] * bias_l[j], compared as fp32.  MILE_CANON_KEY_NORM: bias^2 + sum_i kernel_l[i][j]^2 in
 *         fp64, the terms added one after another, bias first, then i ascending (squares of fp32 values are exact in fp64, so
 *         the key is reproducible bit for bit).
 *   order ascending key; equal keys (-0.0 == +0.0, duplicated units) keep their index order; NaN keys come after every
 *         number, among themselves in index order; +-inf sort as numbers.  p_l[j'] is the original index of the unit that
 *         lands at position j'.
 *   out [M][d] (device, required, not overlapping theta):
 *         bias_l'[j'] = s_l[p_l[j']] * bias_l[p_l[j']]
 *         kernel_l'[i'][j'] = s_{l-1}[p_{l-1}[i']] * s_l[p_l[j']] * kernel_l[p_{l-1}[i']][p_l[j']]
 *         (row factors: identity for l = 0; column factors: identity for the output layer).  Every output float is an input
 *         float moved, possibly negated: nothing is recomputed.  A draw is handled on its own (a NaN in one draw touches no
 *         other), and a draw gives the same bits whatever M is.  With n_layers == 1, H = 0 and out is a copy.
 *   perm [M][H] int32 (device, or null): perm[m][o_l + j'] = p_l[j'].  sign [M][H] int8 (or null): s_l[p_l[j']].
 * Out of scope: the positive rescaling symmetry of ReLU, sigmoid's reflection (it needs a bias correction downstream),
 * alignment to a reference draw by assignment (mile_align_fcn below), and every model other than the FCN.
 * MILE_ERR_INVALID, with nothing launched and no device touched: a null spec, theta or out; M < 1 (or > 2^31 - 1); a model
 * other than MILE_MODEL_FCN, use_bias != 1, or a spec mile_create would refuse; unknown bits in `how`; MILE_CANON_SIGN with an
 * activation other than tanh; a hidden width above MILE_CANON_WIDTH_MAX; out overlapping theta.  MILE_ERR_STATE: a workspace
 * below mile_canonicalize_fcn_workspace's figure -- 0 while a draw with its keys fits the LDS of a compute unit (one launch),
 * 4 * M * H bytes for the row-tiled form of larger draws (two launches); -1 for a bad shape.  mile_canonical_hidden: H, -1 for
 * a bad spec.  Every refusal leaves its message in mile_last_error.
 * (Added under ABI 10: three new symbols, no struct or existing entry changed.) */
int32_t mile_canonicalize_fcn(const mile_model_spec *spec, const float *theta, int64_t M, uint32_t how,
                              float *out, int32_t *perm, int8_t *sign,
                              void *workspace, int64_t workspace_bytes, void *stream);
int64_t mile_canonicalize_fcn_workspace(const mile_model_spec *spec, int64_t M, uint32_t how);
int64_t mile_canonical_hidden(const mile_model_spec *spec);

/* `how` of mile_align_fcn: 0, or the sign fix. */
#define MILE_ALIGN_SIGN      1u
#define MILE_ALIGN_WIDTH_MAX 128

/* Alignment of FCN draws to a reference draw by hidden-unit assignment (re-basin): every draw's hidden units are matched to
 * those of ONE reference row by a linear assignment problem per hidden layer, so that "parameter j" is the same unit in every
 * draw and chain -- an alignment to a mode, where mile_canonicalize_fcn's ordering by a key gives order statistics whose labels
 * switch wherever two keys cross.  Needs no mile_sampler; launches on the current device.
 * theta [M][d] fp32 (device) draws and reference [d] fp32 (device) one row, both of the MILE_MODEL_FCN `spec` in the library's
 * full layout (mile_param_offsets: "layer10" before "layer2").  Hidden layers l = 0 .. n_hidden - 1 (n_hidden = n_layers - 1),
 * widths W_l, the H axis and its spans [o_l, o_l + W_l) as for mile_canonicalize_fcn.  Inputs and outputs never move.  The
 * layers are solved in ascending order (a forward sweep); fin is the fan-in of layer l.
 *   features    reference unit i: (bias^r_l[i], kernel^r_l[0][i], .., kernel^r_l[fin-1][i]).  Draw unit j: (bias_l[j],
 *               s_{l-1}[t] * kernel_l[p_{l-1}[t]][j] for t = 0 .. fin-1) -- the rows already in the previous layer's aligned
 *               order and sign (the identity for l = 0).  For the LAST hidden layer both vectors also carry the unit's outgoing
 *               row kernel_{l+1}[unit][0 .. O-1] (the outputs are never permuted).
 *   similarity  S[i][j]: the dot product of the two vectors in fp64, starting from the bias product, the terms added one after
 *               another in the order above.  Products of fp32 values are exact in fp64, so fused and unfused multiply-adds
 *               round alike: S is reproducible bit for bit.
 *   gain        G = S; with MILE_ALIGN_SIGN (MILE_ACT_TANH only) G = |S|.
 *   assignment  the permutation p_l (reference position i <- draw unit p_l[i]) that maximises sum_i G[i][p_l[i]], found on the
 *               cost c = -G by the shortest-augmenting-path Hungarian method with potentials u (rows), v (columns) in fp64, in
 *               this operation order: rows are inserted in ascending i; inside an augmentation from the row i0 of the column
 *               reached last, cur = (c[i0][j] - u[i0]) - v[j] for every unused column j, minv[j] and way[j] are updated on
 *               cur < minv[j]; the next column is the unused one with the smallest minv, the lowest index among equals, delta
 *               its minv; then u[p[j]] += delta and v[j] -= delta on the used columns (the row being inserted counts as used),
 *               minv[j] -= delta on the others; the augmentation ends at a column without a row and the path is flipped.
 *               Only additions, subtractions and comparisons: the result is the same permutation on every machine.
 *   sign        with MILE_ALIGN_SIGN s_l[i] = -1 iff S[i][p_l[i]] < 0 (zero and NaN are not flipped), else s_l = +1.
 *   score [M][n_hidden] fp64 (device, or null): score[m][l] = sum_i G[i][p_l[i]], added in ascending i from 0.
 *   non-finite  a draw for which any entry of any layer's S is not finite is copied unchanged: perm the identity, sign +1,
 *               its scores NaN, dropped[m] = 1 (dropped [M] int32, device, or null; 0 for every other draw).  The solver never
 *               sees a NaN.  A non-finite reference drops every draw.
 *   out [M][d] (device, required, overlapping neither theta nor reference): exactly mile_canonicalize_fcn's formula with these
 *               p_l and s_l (s_l[i] the sign of position i): bias_l'[i] = s_l[i] * bias_l[p_l[i]], kernel_l'[t][i] =
 *               s_{l-1}[t] * s_l[i] * kernel_l[p_{l-1}[t]][p_l[i]].  Every output float is an input float moved, possibly
 *               negated.  A draw is handled on its own and gives the same bits whatever M is.  With n_layers == 1 out is a copy.
 *   perm [M][H] int32 (or null): perm[m][o_l + i] = p_l[i].  sign [M][H] int8 (or null): s_l[i].
 * Out of scope: refinement of inner layers with their outgoing weights, activation matching, ReLU rescaling, sigmoid's
 * reflection, hidden widths above MILE_ALIGN_WIDTH_MAX, every model other than the FCN.
 * MILE_ERR_INVALID, with nothing launched and no device touched: a null spec, theta, reference or out; M < 1 (or > 2^31 - 1);
 * a model other than MILE_MODEL_FCN, use_bias != 1, or a spec mile_create would refuse; unknown bits in `how`; MILE_ALIGN_SIGN
 * with an activation other than tanh; a hidden width above MILE_ALIGN_WIDTH_MAX; out overlapping theta or reference.
 * MILE_ERR_STATE: a workspace below mile_align_fcn_workspace's figure, 4 * M * H bytes (the rank words that drive the move);
 * -1 for a bad shape.  Every refusal leaves its message in mile_last_error.
 * (Added under ABI 10: two new symbols, no struct or existing entry changed.) */
int32_t mile_align_fcn(const mile_model_spec *spec, const float *theta, int64_t M, const float *reference, uint32_t how,
                       float *out, int32_t *perm, int8_t *sign, double *score, int32_t *dropped,
                       void *workspace, int64_t workspace_bytes, void *stream);
int64_t mile_align_fcn_workspace(const mile_model_spec *spec, int64_t M, uint32_t how);

/* Function-space chain diagnostics: the statistics of mile_chain_diagnostics of what the draws PREDICT, streamed -- the
 * [C][S][N][O] outputs are never held.  Hidden-unit permutations and other symmetries of the parameters leave these series
 * untouched, so their R-hat answers whether the chains agree in their predictions, and their ESS how many effective draws
 * stand behind each.  theta [C*S][d] full layout, draw j of chain c at row c*S + j, as for mile_lppd_stream; X, y as for
 * mile_pointwise_loglik; y may be null.
 * Columns: O the width of the last layer, Q = O + (y ? 1 : 0); column m = n*Q + q is quantity q of row n.  Regression: q = 0
 * mu, q = 1 log sigma, the floats mile_predict writes; q = 2 the row's log-likelihood.  Classification (O <= 64): q = k the fp32
 * softmax probability expf(z_k - (m + logf(se))) with the maximum m and the sum se of the likelihood head; q = O the row's
 * log-likelihood.  With y one last column m = N*Q holds L, the draw's log-likelihood summed in fp64 over the rows in row
 * order (so it does not depend on the tiles) and rounded to fp32 for the statistics.  M = N*Q + (y ? 1 : 0).
 * Outputs (device, null where not asked for): wcv, bcv, rhat [M]; ess, crhat [C][M], by the bits of `what` exactly as in
 * mile_chain_diagnostics with d := M, with its NaN and tie rules; columns [M][C][S] fp32, the series themselves; loglik_sum
 * [C][S] fp64, L before rounding; summary [16] fp64 over the N*Q per-row columns (L's own statistics are at index M - 1 of
 * the arrays), in this order: max rhat, mean rhat, column of the max, columns with rhat above 1.01, 1.05, 1.1, non-finite
 * rhat cells skipped; max crhat, its chain, its column, cells skipped; min ess, mean ess, chain and column of the min, cells
 * skipped (of equal extremes the lower chain, then the lower column; -1 and NaN where no cell is finite); chain_summary
 * [C][2] fp64: each chain's min ess and max crhat.  summary and chain_summary need ESS, CRHAT and RHAT in `what`.
 * Rows go in tiles of at most max_rows_per_tile (0: the library's choice), the forward of a tile in passes of at most
 * max_draws_per_pass draws (0: the library's choice); no output depends on either, bit for bit.
 * MILE_ERR_INVALID, with nothing launched: a null s, theta or X; C outside [1, 65535], S outside [MILE_DIAG_S_MIN,
 * MILE_DIAG_S_MAX], N outside [1, 2^30 - 1]; more than 64 head outputs; n_splits as in mile_chain_diagnostics; unknown bits
 * or MILE_DIAG_POOLED_INPUT in `what`; nothing asked for; a null pointer for a statistic in `what`, a pointer for one that
 * is not; loglik_sum without y; negative caps; ESS / RHAT with C*S > MILE_DIAG_POOL_MAX ("unsupported": WCV, BCV, CRHAT,
 * columns and loglik_sum run at any C*S -- rank the columns outside and pass the scores to mile_chain_diagnostics).
 * mile_function_diagnostics_workspace: the bytes of the workspace kept in the handle for the library's own tile; -1 out of
 * range.  (Added under ABI 10: two new symbols, no struct or existing entry changed.) */
int32_t mile_function_diagnostics(mile_sampler *s, const float *theta, int32_t C, int32_t S, const void *X, const void *y, int64_t N,
                                  int32_t n_splits, uint32_t what, float *wcv, float *bcv, float *ess, float *crhat, float *rhat,
                                  float *columns, double *loglik_sum, double *summary, double *chain_summary,
                                  int64_t max_draws_per_pass, int64_t max_rows_per_tile, void *stream);
int64_t mile_function_diagnostics_workspace(const mile_sampler *s, int32_t C, int32_t S, int64_t N, int32_t with_y);

/* Which outputs mile_chain_diagnostics_tail computes (`what`), and how it reads its input. */
#define MILE_DTAIL_ESS_BULK 1u
#define MILE_DTAIL_ESS_TAIL 2u
#define MILE_DTAIL_ESS_MEAN 4u      /* ess_mean and mcse_mean */
#define MILE_DTAIL_RHAT_FOLDED 8u
#define MILE_DTAIL_PLANE_INPUT 16u  /* samples are [d][C][S] (the `columns` of mile_function_diagnostics): no transpose */

/* Tail diagnostics of the ensemble (Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021): the POOLED effective sample size
 * of the bulk, of the 5 % / 95 % tails and of the mean, the Monte Carlo standard error of the posterior mean, and the split
 * R-hat of the draws folded about their median, which sees chains that agree in location and differ in scale.  Needs no
 * model; launches on the current device.  This comment is the one statement of the definitions.
 * One column has draws x[c][s] (fp32), n = C*S, len = S / n_splits and M = C * n_splits pieces x.reshape(M, len).
 *   order statistics, of the pooled sorted fp32 draws xs[0..n), integer indices only:
 *         q_lo = xs[(n + 19) / 20 - 1]            (index ceil(n / 20) - 1)
 *         q_hi = xs[(19 * n + 19) / 20 - 1]       (index ceil(19 n / 20) - 1)
 *         m32  = fl32((double(xs[(n - 1) / 2]) + double(xs[n / 2])) / 2)
 *         quantiles [3][d] holds q_lo, q_hi, m32 in this order: the draws themselves, bit for bit.
 *   series z: the pooled normal scores of x, ranked as for mile_chain_diagnostics (ties get their average rank);
 *         I_lo = (x <= q_lo), I_hi = (x <= q_hi) as 0 / 1;  x itself;
 *         zf: the pooled normal scores of the folded draws f = |x - m32|, the subtraction in fp32.
 *   ESS_mc(v), the multi-chain estimator of Stan and blackjax on the M pieces, all in fp64:
 *         mean_acov[k]  the mean over the pieces of the biased autocovariance at lag k about the piece's own mean
 *         mean_var0     mean_acov[0] * len / (len - 1)
 *         weighted_var  mean_acov[0] + the ddof-1 variance of the M piece means (that term only when M > 1)
 *         rho_k         1 - (mean_var0 - mean_acov[k]) / weighted_var, rho_0 = 1
 *         Geyer's initial positive and initial monotone sequences on the pairs rho_2t + rho_2t+1, t < floor(len / 2), as in
 *         the single-chain estimator of mile_chain_diagnostics; tau floored at 1 / log10(n); ESS_mc = n / tau.
 *         A weighted_var that is not a positive finite number (a series constant over all pooled draws, a non-finite draw)
 *         gives NaN.
 *   outputs (device, fp32 [d], null where not asked for):
 *         ess_bulk = ESS_mc(z);  ess_tail = min(ESS_mc(I_lo), ESS_mc(I_hi)), NaN if either is;  ess_mean = ESS_mc(x);
 *         mcse_mean = sd / sqrt(ess_mean), sd the ddof-1 standard deviation of the n draws in fp64;
 *         rhat_folded: the pooled split R-hat of mile_chain_diagnostics (its kernels, no other arithmetic) on zf.
 *         A NaN draw makes every output of its column NaN, and its quantiles.  quantiles may be null.
 * Every sum is added in a fixed order, without atomics: the outputs are bitwise reproducible and do not depend on how the
 * parameters were walked in chunks of the workspace.
 * MILE_ERR_INVALID, with nothing launched: null samples; C outside [1, 65535], S outside [MILE_DIAG_S_MIN, MILE_DIAG_S_MAX],
 * d < 1; n_splits < 1 or not a divisor of S, S / n_splits < 2; no statistic or unknown bits in `what`; a null pointer for an
 * output asked for (MILE_DTAIL_ESS_MEAN needs ess_mean and mcse_mean); and, "unsupported", C*S > MILE_DIAG_POOL_MAX with
 * anything that needs the pooled sort: ESS_BULK, ESS_TAIL, RHAT_FOLDED or quantiles (sort those outside and pass the series
 * to mile_multichain_ess, zf to mile_chain_diagnostics with MILE_DIAG_RHAT | MILE_DIAG_POOLED_INPUT).  MILE_ERR_STATE, with
 * nothing launched: a workspace below that of min(d, 32) parameters.  mile_chain_diagnostics_tail_workspace: the size that
 * lets the call run in the fewest launches it will use; -1 for a bad shape.
 *
 * mile_multichain_ess: ESS_mc of m given series, no ranking, at any C*S in the shape range above.  series [C][S][m] fp32, or
 * [m][C][S] with plane_input != 0 (then no workspace is needed and its size is 0); ess [m] fp32.  The same errors: null
 * series or ess, the shape (m for d), n_splits, a workspace below min(m, 32) series.
 * (Added under ABI 10: four new symbols, no struct or existing entry changed.) */
int32_t mile_chain_diagnostics_tail(const float *samples, int32_t C, int32_t S, int64_t d, int32_t n_splits, uint32_t what,
                                    float *ess_bulk, float *ess_tail, float *ess_mean, float *mcse_mean, float *rhat_folded,
                                    float *quantiles, void *workspace, int64_t workspace_bytes, void *stream);
int64_t mile_chain_diagnostics_tail_workspace(int32_t C, int32_t S, int64_t d, uint32_t what);
int32_t mile_multichain_ess(const float *series, int32_t C, int32_t S, int64_t m, int32_t n_splits, int32_t plane_input,
                            float *ess, void *workspace, int64_t workspace_bytes, void *stream);
int64_t mile_multichain_ess_workspace(int32_t C, int32_t S, int64_t m, int32_t plane_input);

/* Input sensitivities of the ensemble's predictions: which inputs drive the prediction, in which direction, and whether the
 * posterior is sure of it.  MILE_MODEL_FCN only.  With a_0 = x, z_l = a_l W_l + b_l, a_{l+1} = phi(z_l) for l < L - 1 and the raw
 * outputs r = z_{L-1}, the Jacobian of draw s on row n is
 *   Jraw[o][f] = d r_o / d x_f = [W_0 diag phi'(z_0) W_1 ... diag phi'(z_{L-2}) W_{L-1}]_{f,o},
 * phi' as the gradient kernels take it (relu' = 1 iff z > 0), formed in fp32 by one forward and P backward sweeps (k_sens_jac,
 * mile_sens.h).  The reported columns J[p][f], P = the width of the last layer:
 *   regression, P = 2:   J = Jraw: the sensitivities of mu and of log sigma, unclipped, as mile_predict returns them
 *   K classes, P = K:    J[k][f] = pi_k (Jraw[k][f] - sum_j pi_j Jraw[j][f]), the sensitivities of the class probabilities
 *                        pi = softmax(r) (maximum subtracted first, as in the likelihood head); logit Jacobians are not reported
 * theta [C * S, d] full layout, draw j of chain c at row c * S + j; X [N, F] any device table, as for mile_predict.
 * A (draw, row) pair is kept iff its raw outputs and all P * F entries of J are finite; otherwise it is left out of that row (per
 * draw and per row, the rule of mile_predict_moments).  A NaN pre-activation stays NaN in this forward for every activation
 * (the ReLU of the evaluation kernels answers 0 for it), so a NaN weight or an inf - inf inside the net drops the pair by its raw
 * outputs.  Outputs (device, any may be null, not all):
 *   mean, sd, pos [N, P, F] fp32   over the k kept draws of all chains on the row: the mean of J, sd = sqrt(M2 / (k - 1)) (0 for
 *                                  k = 1: the epistemic spread of the effect) and the share of kept draws with J > 0; a row with
 *                                  nothing kept holds NaN
 *   dropped [N] int32              C * S - k
 *   chain_ape, chain_abs [C, P, F] fp64   over chain c's kept (draw, row) pairs: the mean of J (the average partial effect) and of
 *                                  |J| (the importance); NaN for a chain with nothing kept
 *   chain_kept [C] int64           those pairs
 * Rows go in tiles of at most max_rows_per_tile (0: the library's choice), the draws of a tile in passes of at most
 * max_draws_per_pass (0: as many as fit 256 MiB of Jacobians) -- never [C * S, N, P, F] at once.  Accumulators are fp64: Welford
 * per pass with Chan's merge across passes on the draw axis, two-stage sums in a fixed order over rows; no atomics: the outputs
 * are bitwise reproducible for one (C, S, N, max_draws_per_pass, max_rows_per_tile) and agree across them to fp64 rounding.
 * The workspace is the handle's shared evaluation workspace (see mile_predict_moments), grown in the call;
 * mile_predict_sensitivities_workspace gives its bytes with the library's tile and pass, -1 where the call would be refused.
 * MILE_ERR_INVALID, with nothing launched and the handle usable: a null handle / theta / X; C outside [1, 1024], S < 1,
 * C * S > 2^31 - 1, N outside [1, 2^30 - 1]; negative caps; no output; an output that overlaps theta or X; a model other than
 * MILE_MODEL_FCN (token ids and image pixels are out of scope); a network one row of which does not fit 160 KiB of LDS.
 * MILE_ERR_NOMEM: the workspace.  (Added under ABI 10: two new symbols, no struct or existing entry changed.) */
int32_t mile_predict_sensitivities(mile_sampler *s, const float *theta, int32_t C, int64_t S, const void *X, int64_t N,
                                   int64_t max_draws_per_pass, int64_t max_rows_per_tile, float *mean, float *sd, float *pos,
                                   int32_t *dropped, double *chain_ape, double *chain_abs, int64_t *chain_kept, void *stream);
int64_t mile_predict_sensitivities_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N);

/* Partial dependence (Friedman 2001) and ICE curves (Goldstein et al. 2015) of the ensemble's predictions: how the prediction
 * moves when one input runs over a grid, whether the posterior is sure of that curve, and whether the chains agree on it.
 * MILE_MODEL_FCN only.  The head columns are those of mile_predict_sensitivities: regression P = 2, mu and log sigma, unclipped;
 * K classes P = K, the softmax probabilities (maximum subtracted first).  For draw s, row n, the selected feature f = features[i]
 * and the grid value v = grid[i][g],
 *   h[s, n, i, g, p] = head column p of the FCN on row n with x_{n,f} replaced by v,
 * computed in fp32 as z_0 = x W_0 + b_0 once per (draw, row), z_0' = z_0 + (v - x_{n,f}) W_0[f, :] (one fmaf per first-layer unit)
 * per grid value, then the activation, the layers 1 .. L - 1 and the head (k_pdp_fwd, mile_pdp.h).  This arithmetic is the
 * definition; in exact arithmetic it is the substitution.  A NaN pre-activation stays NaN, as for the sensitivities.
 * A (draw, row, feature) triple is kept iff all G * P values of the feature are finite -- per feature on purpose: columns of
 * different features are independent, and a call on a subset of the features returns, for those, the bits of the full call.
 * A row with a non-finite input is dropped for EVERY feature, the feature of that column included: z_0 already holds the inf,
 * and z_0 + (v - inf) W_0[f, :] is NaN (true substitution would have kept that one feature).
 * theta [C * S, d] full layout, draw j of chain c at row c * S + j; X [N, F] device; features [Fs] a HOST array of distinct
 * indices in [0, F); grid [Fs, G] fp32 device, any values, not necessarily sorted.  Outputs (device, any may be null, not all):
 *   ice_mean, ice_sd [N, Fs, G, P] fp32   over the k kept draws of all chains on (row, feature): the mean of h and
 *                                  sd = sqrt(M2 / (k - 1)) (0 for k = 1); NaN where nothing is kept
 *   dropped [N, Fs] int32          C * S - k
 *   curves [C * S, Fs, G, P] fp32  the draw's partial dependence: the mean of h over its kept rows, rounded from the fp64 sum;
 *                                  NaN for a (draw, feature) with no kept row
 *   pd_mean, pd_sd [Fs, G, P] fp64 mean and sd (ddof 1, 0 for one) over the draws that have a curve, from the fp64 row means and
 *                                  not from the rounded curves: the posterior band; NaN where no draw has one
 *   chain_pd [C, Fs, G, P] fp64    the mean of chain c's curves; NaN for a chain without one
 *   chain_draws [C, Fs] int64      chain c's draws that have a curve
 * Rows go in tiles of at most max_rows_per_tile (0: the library's choice), the draws of a tile in passes of at most
 * max_draws_per_pass (0: as many as fit 256 MiB) -- never [C * S, N, Fs, G, P] at once; tiles and passes are sized as if all F
 * features were selected, so a subset runs the plan of the full call.  Accumulators are fp64: Welford per pass with Chan's merge
 * across passes on the draw axis, two-stage sums in a fixed order over rows, the draws of a chain and then the chains in index
 * order; no atomics: the outputs are bitwise reproducible for one (C, S, N, Fs, G, max_draws_per_pass, max_rows_per_tile) and
 * agree across passes and tiles to fp64 rounding.  The workspace is the handle's shared evaluation workspace, grown in the
 * call; mile_predict_partial_dependence_workspace gives its bytes with the library's tile and pass, -1 where the call would be
 * refused.  MILE_ERR_INVALID, with nothing launched and the handle usable: a null handle / theta / X / features / grid; C outside
 * [1, 1024], S < 1, C * S > 2^31 - 1, N outside [1, 2^30 - 1]; Fs outside [1, F], a feature index out of range or repeated; G
 * outside [1, 256]; negative caps; no output; an output that overlaps theta, X or grid; a model other than MILE_MODEL_FCN; a
 * network of which one row's first layer and one pseudo-row do not fit 160 KiB of LDS; per-draw sums C * S * Fs * G * P * 8 bytes
 * above 1 GiB (call it on fewer features: exact by the drop rule).  MILE_ERR_NOMEM: the workspace.
 * (Added under ABI 10: two new symbols, no struct or existing entry changed.) */
int32_t mile_predict_partial_dependence(mile_sampler *s, const float *theta, int32_t C, int64_t S, const void *X, int64_t N,
                                        const int32_t *features, int32_t Fs, const float *grid, int32_t G,
                                        int64_t max_draws_per_pass, int64_t max_rows_per_tile,
                                        float *ice_mean, float *ice_sd, int32_t *dropped, float *curves,
                                        double *pd_mean, double *pd_sd, double *chain_pd, int64_t *chain_draws, void *stream);
int64_t mile_predict_partial_dependence_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N, int32_t Fs, int32_t G);

/* Partition sampling (sampler.partition_sampling of the reference: src/training/partition_sampling.py:304-315 partition_params,
 * src/training/trainer.py:593-659): only the FIRST and the LAST layer of an FCN are sampled; every other layer keeps, per chain,
 * the values of `frozen`.  Target: log_prior(sampled coordinates only) + log_likelihood(full net on sampled U frozen).
 * frozen [E, d] full-layout rows (d = mile_param_count), COPIED into rows the library owns; their sampled coordinates are
 * overwritten by every gradient call.  Call it before mile_reserve (it drops the workspace); calling it again replaces the
 * rows.  From then on mile_logpost_grad, mile_init, mile_step and mile_tune take and return COMPACT arrays: every [E, d]
 * (theta, grad, the mile_state, noise, sqrt_diag_cov, out_samples; stream_average [E, 2, d]) is [E, d_s], d_s =
 * mile_partition_dim, the sampled segments (mile_partition_segments) concatenated in full-row order, and d_s is the dimension
 * in every formula of the integrator and the tuner.  Philox streams are keyed by the index inside the compact row.  E of those
 * calls must equal the frozen rows' E.  mile_param_count / mile_param_offsets stay full-layout, and so do
 * mile_pointwise_loglik, mile_predict and mile_warmstart_step (give them merged rows).
 * AUTO keeps its choice; where that is MFMA_NARROW_F32 the partition form of k_grad_narrow reads both sources itself, skips the
 * hidden layers' dW / db and writes slabs of width d_s; every other FCN kernel runs unchanged on the library's full rows between
 * a scatter and a gather launch.  An FCN with <= 2 layers has no frozen layer: d_s = d and the ordinary path runs.
 * MILE_ERR_INVALID: a model other than MILE_MODEL_FCN; E < 1; later, E different from the frozen rows', and mile_nuts_*
 * on a handle in partition mode (not built).
 * (Added under ABI 10: three new symbols, no struct or existing entry changed.) */
int32_t mile_set_partition(mile_sampler *s, const float *frozen, int32_t E, void *stream);
/* d_s in partition mode; mile_param_count otherwise. */
int64_t mile_partition_dim(const mile_sampler *s);
/* The sampled segments of the full row in full-row order: begin[i], length[i] for i < the return value (at most 4:
 * layer0.bias|kernel are adjacent, so are the last layer's; lexicographic layer order decides whether the two pairs touch).
 * Null pointers are allowed (count only).  0 segments outside partition mode; negative mile_status on error. */
int32_t mile_partition_segments(const mile_sampler *s, int64_t *begin, int64_t *length, int32_t capacity);

/* Size the NUTS trajectory buffers (ends,momentum sums, proposals, [E, max_num_doublings, d] U-turn checkpoints) for
 * ensembles of up to E chains, and the grad workspace as mile_reserve.  Allocation happens here, never in a launch. */
int32_t mile_nuts_reserve(mile_sampler *s, int32_t E, int32_t max_num_doublings);

/* Replaces: the scan of sampler.step(rng_key, state) with sampler = blackjax.nuts(...) (src/training/sampling.py:140-178,
 * 200-210).  state->position / logdensity / logdensity_grad (HMCState; momentum is not used) advance in place.
 * Synchronises `stream` once per doubling ("how many chains go on"); never per leapfrog. */
int32_t mile_nuts_step(mile_sampler *s, mile_state *state, const mile_nuts_args *a, void *stream);

/* Replaces: the lax.scan of one_step in custom_window_adaptation.run (src/training/warmup.py:89-140): n_steps NUTS steps
 * with the adaptation state's step size and inverse mass matrix, each followed by one on-device adaptation update. */
int32_t mile_nuts_warmup(mile_sampler *s, mile_state *state, const mile_nuts_args *a, const mile_nuts_adapt_args *w,
                         void *stream);

/* Counter-RNG words/normals exactly as the step kernels draw them (test hook). out [E, d]. */
int32_t mile_debug_noise(mile_sampler *s, uint64_t seed, const int32_t *particle_ids, int32_t E,
                         int64_t step, int32_t stage, float *out, void *stream);

/* Test hook: how many mid-step update launches of mile_step have drawn the following record launch's Philox noise
 * (the noise prefill) since mile_create; -1 for a null handle. */
int64_t mile_debug_prefill_count(const mile_sampler *s);

/* Introspection for bench.py's roofline: name, workgroups and LDS bytes of the grad kernel
 * that the current configuration launches for E particles. */
int32_t mile_grad_launch_info(const mile_sampler *s, int32_t E, int32_t *grid_x, int32_t *grid_y,
                              int32_t *block, int32_t *lds_bytes, char *name, int32_t name_len);

/* HIP-event timing of the grad kernel launches only (on `stream`): call begin, run steps,
 * call end -> total milliseconds and number of grad launches in between. */
int32_t mile_grad_timing_begin(mile_sampler *s);
int32_t mile_grad_timing_end(mile_sampler *s, float *total_ms, int32_t *n_launches);

#ifdef __cplusplus
}
#endif
#endif /* MILE_HIP_H_ */
