"""ctypes binding of include/mile_hip.h.  Fails loudly if the HIP library is missing."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

from mile_amd._build import LIB_PATH

MILE_MAX_LAYERS = 16
ABI_VERSION = 10

ACTIVATION_IDS = {'relu': 0, 'tanh': 1, 'sigmoid': 2}
TASK_IDS = {'regr': 0, 'regression': 0, 'classification': 1, 'class': 1}
PRIOR_IDS = {'Normal': 0, 'StandardNormal': 0, 'Laplace': 1}
REFRESH_IDS = {'O-step-O': 0, 'step-O': 1}
GRAD_KERNEL_IDS = {'auto': 0, 'generic': 1, 'mfma_w64': 2, 'mfma_w128_bf16': 3, 'gemm_f32': 4, 'lenet_f32': 5, 'mfma_w64_bf16x3': 6,
                   'mfma_wide_bf16x3': 7, 'mfma_wide_bf16': 8, 'lenet_bf16': 9, 'mfma_narrow_f32': 10,
                   'lenetti_f32': 11, 'attn_f32': 12, 'attn_pre_f32': 13, 'attn_wide_f32': 14, 'lenet_bf16x3': 15}
DIAG_BITS = {'wcv': 1, 'bcv': 2, 'ess': 4, 'crhat': 8, 'rhat': 16, 'pooled_input': 32}     # MILE_DIAG_*
DIAG_S_MIN, DIAG_S_MAX, DIAG_POOL_MAX = 4, 4096, 16384
DTAIL_BITS = {'ess_bulk': 1, 'ess_tail': 2, 'ess_mean': 4, 'rhat_folded': 8, 'plane_input': 16}   # MILE_DTAIL_*
# layout of mile_function_diagnostics' summary (the FDIAG_* enum of csrc/mile_fdiag.h)
FDIAG_SUMMARY = ('rhat_max', 'rhat_mean', 'rhat_column', 'rhat_gt_1_01', 'rhat_gt_1_05', 'rhat_gt_1_1', 'rhat_skipped',
                 'crhat_max', 'crhat_chain', 'crhat_column', 'crhat_skipped',
                 'ess_min', 'ess_mean', 'ess_chain', 'ess_column', 'ess_skipped')
FDIAG_O_MAX = 64
CANON_BITS = {'bias': 0, 'norm': 1, 'sign': 2}                                                # MILE_CANON_*
CANON_WIDTH_MAX = 1024
ALIGN_SIGN = 1                                                                                # MILE_ALIGN_SIGN
ALIGN_WIDTH_MAX = 128
MODEL_IDS = {'fcn': 0, 'lenet': 1, 'lenetti': 2, 'attn': 3, 'attn_pretrained': 4, 'attn_wide': 5}


class ModelSpecC(C.Structure):
    _fields_ = [
        ('in_features', C.c_int32),
        ('n_layers', C.c_int32),
        ('widths', C.c_int32 * MILE_MAX_LAYERS),
        ('activation', C.c_int32),
        ('task', C.c_int32),
        ('prior', C.c_int32),
        ('prior_loc', C.c_float),
        ('prior_scale', C.c_float),
        ('use_bias', C.c_int32),
        ('model', C.c_int32),
        ('img_c', C.c_int32),
        ('img_h', C.c_int32),
        ('img_w', C.c_int32),
        ('vocab_size', C.c_int32),
        ('ctx_len', C.c_int32),
        ('emb_size', C.c_int32),
        ('n_heads', C.c_int32),
        ('qkv_dim', C.c_int32),
    ]


def fcn_spec_c(spec) -> ModelSpecC:
    """The mile_model_spec of an FCN ``mile_amd.spec.ModelSpec``, for the calls that take a spec and no handle."""
    if len(spec.hidden_structure) > MILE_MAX_LAYERS:
        raise ValueError(f'at most {MILE_MAX_LAYERS} layers')
    cs = ModelSpecC()
    cs.in_features = spec.in_features
    cs.n_layers = len(spec.hidden_structure)
    for i, w in enumerate(spec.hidden_structure):
        cs.widths[i] = w
    cs.activation = ACTIVATION_IDS[spec.activation]
    cs.task = TASK_IDS[spec.task]
    cs.prior = PRIOR_IDS[spec.prior]
    cs.prior_loc = spec.prior_loc
    cs.prior_scale = spec.prior_scale
    cs.use_bias = int(spec.use_bias)
    cs.model = MODEL_IDS['fcn']
    return cs


class StateC(C.Structure):
    _fields_ = [
        ('n_particles', C.c_int32),
        ('position', C.c_void_p),
        ('momentum', C.c_void_p),
        ('logdensity', C.c_void_p),
        ('logdensity_grad', C.c_void_p),
    ]


class StepArgsC(C.Structure):
    _fields_ = [
        ('step_size', C.c_void_p),
        ('L', C.c_void_p),
        ('sqrt_diag_cov', C.c_void_p),
        ('noise', C.c_void_p),
        ('seed', C.c_uint64),
        ('particle_ids', C.c_void_p),
        ('step_offset', C.c_int64),
        ('n_steps', C.c_int32),
        ('n_thinning', C.c_int32),
        ('refresh', C.c_int32),
        ('out_samples', C.c_void_p),
        ('out_info', C.c_void_p),
    ]


class TuneArgsC(C.Structure):
    _fields_ = [
        ('step_size', C.c_void_p), ('L', C.c_void_p), ('sqrt_diag_cov', C.c_void_p),
        ('step_size_max', C.c_void_p), ('time', C.c_void_p), ('x_average', C.c_void_p),
        ('stream_weight', C.c_void_p), ('stream_average', C.c_void_p), ('noise', C.c_void_p),
        ('seed', C.c_uint64), ('particle_ids', C.c_void_p), ('step_offset', C.c_int64),
        ('n_steps', C.c_int32), ('schedule_step0', C.c_int32), ('n_mask_steps', C.c_int32),
        ('schedule_total', C.c_int32), ('desired_energy_var_start', C.c_float),
        ('desired_energy_var_end', C.c_float), ('trust_in_estimate', C.c_float), ('decay_rate', C.c_float),
        ('refresh', C.c_int32), ('out_info', C.c_void_p),
    ]


class OptimArgsC(C.Structure):
    _fields_ = [
        ('kind', C.c_int32), ('learning_rate', C.c_float), ('b1', C.c_float), ('b2', C.c_float), ('eps', C.c_float),
        ('weight_decay', C.c_float), ('t', C.c_int64), ('m', C.c_void_p), ('v', C.c_void_p), ('active', C.c_void_p),
        ('out_nll', C.c_void_p),
    ]


OPTIMIZER_IDS = {'sgd': 0, 'adam': 1, 'adamw': 2}


class NutsArgsC(C.Structure):
    _fields_ = [
        ('step_size', C.c_void_p), ('inverse_mass_matrix', C.c_void_p), ('max_num_doublings', C.c_int32),
        ('divergence_threshold', C.c_float), ('momentum_noise', C.c_void_p), ('uniforms', C.c_void_p),
        ('seed', C.c_uint64), ('particle_ids', C.c_void_p), ('step_offset', C.c_int64), ('n_steps', C.c_int32),
        ('n_thinning', C.c_int32), ('out_samples', C.c_void_p), ('out_info', C.c_void_p),
        ('out_stats', C.POINTER(C.c_int64)),
    ]


class NutsAdaptArgsC(C.Structure):
    _fields_ = [
        ('step_size', C.c_void_p), ('inverse_mass_matrix', C.c_void_p), ('da', C.c_void_p), ('welford', C.c_void_p),
        ('welford_count', C.c_void_p), ('schedule', C.POINTER(C.c_int32)), ('target_acceptance_rate', C.c_float),
    ]

# name -> (restype, argtypes): every symbol include/mile_hip.h declares
SIGNATURES = {
    'mile_last_error': (C.c_char_p, []),
    'mile_abi_version': (C.c_int32, []),
    'mile_create': (C.c_int32, [C.POINTER(ModelSpecC), C.c_int32, C.POINTER(C.c_void_p)]),
    'mile_destroy': (C.c_int32, [C.c_void_p]),
    'mile_param_count': (C.c_int64, [C.c_void_p]),
    'mile_param_offsets': (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'mile_set_data': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'mile_set_embedding': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'mile_set_row_window': (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64]),
    'mile_set_partition': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    'mile_partition_dim': (C.c_int64, [C.c_void_p]),
    'mile_partition_segments': (C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]),
    'mile_reserve': (C.c_int32, [C.c_void_p, C.c_int32]),
    'mile_slab_bytes': (C.c_int64, [C.c_void_p]),
    'mile_warmstart_step': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(OptimArgsC), C.c_void_p]),
    'mile_set_grad_kernel': (C.c_int32, [C.c_void_p, C.c_int32]),
    'mile_get_grad_kernel': (C.c_int32, [C.c_void_p]),
    'mile_logpost_grad': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'mile_init': (C.c_int32, [C.c_void_p, C.POINTER(StateC), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    'mile_step': (C.c_int32, [C.c_void_p, C.POINTER(StateC), C.POINTER(StepArgsC), C.c_void_p]),
    'mile_tune': (C.c_int32, [C.c_void_p, C.POINTER(StateC), C.POINTER(TuneArgsC), C.c_void_p]),
    'mile_pointwise_loglik': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.c_void_p, C.c_void_p]),
    'mile_predict': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    'mile_predict_moments': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_void_p]),
    'mile_predict_moments_width': (C.c_int32, [C.c_void_p]),
    'mile_lppd_stream': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p]),
    'mile_lppd_stream_workspace': (C.c_int64, [C.c_void_p, C.c_int32, C.c_int64]),
    'mile_mixture_quantiles': (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    'mile_predict_quantiles': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'mile_predict_quantiles_workspace': (C.c_int64, [C.c_void_p, C.c_int64, C.c_int64]),
    'mile_mixture_quantiles_weighted': (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'mile_predict_quantiles_weighted': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                                    C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                    C.c_int64, C.c_void_p]),
    'mile_predict_quantiles_weighted_workspace': (C.c_int64, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64]),
    'mile_debug_quantile_sweeps': (C.c_int32, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    'mile_psis_loo': (C.c_int32, [C.c_void_p, C.c_int64, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    'mile_loo_stream': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'mile_loo_stream_workspace': (C.c_int64, [C.c_void_p, C.c_int64, C.c_int64]),
    'mile_chain_loo_stream': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_double,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'mile_chain_loo_stream_workspace': (C.c_int64, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64]),
    'mile_psis_expect': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'mile_loo_predict_stream': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                            C.c_void_p]),
    'mile_loo_predict_stream_workspace': (C.c_int64, [C.c_void_p, C.c_int64, C.c_int64]),
    'mile_stack_eval': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int64, C.c_void_p]),
    'mile_mixture_crps': (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'mile_crps_stream': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_int64, C.c_void_p]),
    'mile_crps_stream_workspace': (C.c_int64, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64]),
    'mile_calibration': (C.c_int32, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    'mile_calibration_stream': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'mile_calibration_stream_workspace': (C.c_int64, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64]),
    'mile_chain_diagnostics': (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'mile_chain_diagnostics_workspace': (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_uint32]),
    'mile_function_diagnostics': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                              C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'mile_function_diagnostics_workspace': (C.c_int64, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    'mile_chain_diagnostics_tail': (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_uint32, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                C.c_void_p]),
    'mile_chain_diagnostics_tail_workspace': (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_uint32]),
    'mile_multichain_ess': (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_int64, C.c_void_p]),
    'mile_multichain_ess_workspace': (C.c_int64, [C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    'mile_predict_sensitivities': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
    'mile_predict_sensitivities_workspace': (C.c_int64, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64]),
    'mile_predict_partial_dependence': (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64,
                                                    C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_int64,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p]),
    'mile_predict_partial_dependence_workspace': (C.c_int64, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    'mile_canonicalize_fcn': (C.c_int32, [C.POINTER(ModelSpecC), C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int64, C.c_void_p]),
    'mile_canonicalize_fcn_workspace': (C.c_int64, [C.POINTER(ModelSpecC), C.c_int64, C.c_uint32]),
    'mile_canonical_hidden': (C.c_int64, [C.POINTER(ModelSpecC)]),
    'mile_align_fcn': (C.c_int32, [C.POINTER(ModelSpecC), C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'mile_align_fcn_workspace': (C.c_int64, [C.POINTER(ModelSpecC), C.c_int64, C.c_uint32]),
    'mile_debug_noise': (C.c_int32, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int32, C.c_int64, C.c_int32,
                                     C.c_void_p, C.c_void_p]),
    'mile_debug_prefill_count': (C.c_int64, [C.c_void_p]),
    'mile_grad_launch_info': (C.c_int32, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_char_p, C.c_int32]),
    'mile_nuts_reserve': (C.c_int32, [C.c_void_p, C.c_int32, C.c_int32]),
    'mile_nuts_step': (C.c_int32, [C.c_void_p, C.POINTER(StateC), C.POINTER(NutsArgsC), C.c_void_p]),
    'mile_nuts_warmup': (C.c_int32, [C.c_void_p, C.POINTER(StateC), C.POINTER(NutsArgsC), C.POINTER(NutsAdaptArgsC),
                                     C.c_void_p]),
    'mile_grad_timing_begin': (C.c_int32, [C.c_void_p]),
    'mile_grad_timing_end': (C.c_int32, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
}

_lib = None


class MileHipError(RuntimeError):
    pass


def load_library(path: str | Path | None = None) -> C.CDLL:
    """dlopen libmile_hip.so.  There is NO fallback: without the HIP library the product
    path cannot run, and says so."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise MileHipError(
            f'{p} not found: the MI355X HIP extension is not built. Run '
            '`python -c "import __graft_entry__ as g; g.build()"` (needs hipcc). '
            'mile_amd has no CPU fallback.')
    try:
        lib = C.CDLL(str(p))
    except OSError as exc:
        raise MileHipError(f'cannot load {p}: {exc}') from exc
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise MileHipError(f'{p} does not export {name}') from exc
        fn.restype = res
        fn.argtypes = args
    if lib.mile_abi_version() != ABI_VERSION:
        raise MileHipError(f'ABI mismatch: library {lib.mile_abi_version()} != binding {ABI_VERSION}')
    if path is None:
        _lib = lib
    return lib


def check(rc: int, lib: C.CDLL | None = None):
    if rc != 0:
        lib = lib or load_library()
        msg = lib.mile_last_error()
        raise MileHipError(f'libmile_hip error {rc}: {msg.decode() if msg else "?"}')
