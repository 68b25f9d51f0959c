#!/usr/bin/env python3
"""LPPD, ACC, RMSE, coverage and calibration error of a finished experiment (the consumer of mile_pointwise_loglik and
mile_predict; mirrors what the reference's report notebook does with src/inference/evaluation.py:409-544 +
src/inference/metrics.py:247-312):

    python evaluate.py -e results/mile_amd/<experiment> [--split test] [--diagnostics [N_SPLITS]] [--function-diagnostics [N_SPLITS]] [--canonical-diagnostics [N_SPLITS]] [--aligned-diagnostics [N_SPLITS]] [--tail-diagnostics [N_SPLITS]] [--moments] [--sensitivities] [--partial-dependence [G]] [--pd-features I ..] [--running [N_POINTS]] [--intervals] [--loo] [--loo-predict] [--stacking]

Reloads config.yaml and the samples/<chain>/sample_<n>.npz files, rebuilds the data split with the same
seed, evaluates all C x S samples on the split in one device pass and writes metrics.json next to them.
"""
import argparse
import json
from pathlib import Path

import numpy as np
import torch


def sample_chunk(N, O, budget=1 << 30):
    """Samples per Engine.predict call: the raw block [chunk, N, O] fp32 stays under ``budget`` bytes."""
    return max(1, (budget - 1) // (N * O * 4))


def predictive_metrics(eng, samples, x, y, task, seed, coverages, with_rmse=True, budget=1 << 30):
    """The part of evaluate_bde's report that needs the raw outputs (src/inference/evaluation.py:459-543): ACC for
    classification; coverage, calibration error and (``with_rmse``) RMSE for regression.  samples [C, S, d] (host).

    The samples are walked chain by chain in chunks of ``sample_chunk`` through Engine.predict, and each chunk's draws come
    from ONE device generator seeded ``seed``, in that order.  Only the class counts [C, N, K], or the draws [C, S, N], are
    kept -- never the raw outputs of the whole experiment."""
    from mile_amd import metrics as M
    dev = eng.device
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    C_, S_, N = samples.shape[0], samples.shape[1], x.shape[0]
    O = eng.spec.hidden_structure[-1]
    xt = torch.from_numpy(x).to(dev)
    step = sample_chunk(N, O, budget)
    res = {}
    if task != 'regr':
        yt = torch.from_numpy(y).to(dev).reshape(-1)
        counts = torch.zeros((C_, N, O), dtype=torch.int64, device=dev)
        for c in range(C_):
            for s0 in range(0, S_, step):
                raw = eng.predict(torch.from_numpy(samples[c, s0:s0 + step]), xt)
                counts[c] += M.class_counts(M.sample_from_predictions(raw, task, gen), O)
        pc = M.accuracy_from_counts(counts, yt)
        res['acc'] = float(M.accuracy_from_counts(counts.sum(dim=0), yt).item())
        res['per_chain_acc'] = [float(v) for v in pc.cpu()]
        res['per_chain_acc_median'] = float(pc.median().item())
        return res
    yt = torch.from_numpy(y).to(dev).to(torch.float32).reshape(-1)
    draws = torch.empty((C_, S_, N), dtype=torch.float32, device=dev)
    mu_sum = torch.zeros(N, dtype=torch.float64, device=dev)
    mu_chain = torch.zeros((C_, N), dtype=torch.float64, device=dev)
    n_ok = 0
    for c in range(C_):
        for s0 in range(0, S_, step):
            raw = eng.predict(torch.from_numpy(samples[c, s0:s0 + step]), xt)
            draws[c, s0:s0 + step] = M.sample_from_predictions(raw, task, gen)
            mu = raw[..., 0]
            fin_rows = torch.isfinite(mu).all(dim=1)                 # (the FCN rmse above: samples with a finite prediction)
            mu_sum += mu[fin_rows].double().sum(dim=0)
            n_ok += int(fin_rows.sum())
            mu_chain[c] += torch.nan_to_num(mu.double(), nan=0.0, posinf=0.0, neginf=0.0).sum(dim=0)
    if with_rmse and n_ok:
        res['rmse'] = float(torch.sqrt(((yt.double() - mu_sum / n_ok) ** 2).mean()).item())
        rc = torch.sqrt(((yt.double()[None] - mu_chain / S_) ** 2).mean(dim=1))
        res['per_chain_rmse'] = [float(v) for v in rc.cpu()]
        res['per_chain_rmse_median'] = float(rc.median().item())
    # chains with a non-finite draw are left out, as the reference leaves out its NaN chains (evaluation.py:493-497,532)
    ok = torch.isfinite(draws).all(dim=2).all(dim=1)
    if bool(ok.any()):
        cov = M.calculate_coverage(coverages, yt, draws[ok])
        for c, v in zip(coverages, cov.cpu()):
            res[f'coverage_{c}'] = float(v)
        res['cal_error'] = float(M.calibration_error(coverages, cov).item())
    return res


def diagnostic_metrics(samples, spec, n_splits, device):
    """--diagnostics: ESS, split R-hat and within / between chain variance of EVERY parameter of the finite chains
    (mile_amd.metrics.chain_diagnostics; the reference's experiments/diagnostics + plot_effective_sample_size /
    plot_split_chain_r_hat, src/visualization/samples.py:158-212).  samples [C, S, d] (host).  Returns the metrics.json
    keys and the full arrays for diagnostics.npz; ({}, None) without the flag (``n_splits`` None)."""
    if n_splits is None:
        return {}, None
    from mile_amd.metrics import chain_diagnostics
    fin = np.isfinite(samples).all(axis=(1, 2))
    ok = np.ascontiguousarray(samples[fin])
    if ok.shape[0] == 0:
        raise SystemExit('--diagnostics: no chain with finite samples')
    res = chain_diagnostics(torch.from_numpy(ok).to(device), n_splits)
    arr = {k: v.detach().cpu().numpy() for k, v in res.items()}
    return diagnostic_keys('diag', arr, spec, n_splits), arr


def diagnostic_keys(prefix, arr, spec, n_splits):
    """The metrics.json keys of the five per-parameter arrays ``arr`` under ``prefix`` (diag: the draws as sampled; cdiag: their
    canonical ordering)."""
    out = {f'{prefix}_n_splits': int(n_splits),
           f'{prefix}_ess_min': float(np.nanmin(arr['ess'])), f'{prefix}_ess_median': float(np.nanmedian(arr['ess'])),
           f'{prefix}_crhat_median': float(np.nanmedian(arr['crhat'])), f'{prefix}_crhat_max': float(np.nanmax(arr['crhat'])),
           f'{prefix}_rhat_median': float(np.nanmedian(arr['rhat'])), f'{prefix}_rhat_max': float(np.nanmax(arr['rhat'])),
           f'{prefix}_wcv_median': float(np.nanmedian(arr['wcv'])), f'{prefix}_bcv_median': float(np.nanmedian(arr['bcv']))}
    # per-layer means, keyed by leaf name as plot_effective_sample_size / plot_split_chain_r_hat return them
    for key in ('ess', 'crhat'):
        out[f'{prefix}_{key}_layer_mean'] = {name: float(np.mean(arr[key][:, off:off + int(np.prod(shape))]))
                                             for name, off, shape in spec.leaves()}
    return out


def tail_diagnostic_metrics(samples, n_splits, device):
    """--tail-diagnostics: the pooled bulk / tail / mean ESS, the MCSE of the mean and the folded split R-hat of EVERY parameter of
    the finite chains (mile_amd.metrics.tail_diagnostics: mile_chain_diagnostics_tail on the device).  samples [C, S, d] (host).
    Returns the dtail_* keys of metrics.json and the arrays of tail_diagnostics.npz."""
    from mile_amd import metrics as M
    fin = np.isfinite(samples).all(axis=(1, 2))
    ok = np.ascontiguousarray(samples[fin])
    if ok.shape[0] == 0:
        raise SystemExit('--tail-diagnostics: no chain with finite samples')
    xt = torch.from_numpy(ok).to(device)
    res = M.tail_diagnostics(xt, n_splits)
    rhat = M.chain_diagnostics(xt, n_splits)['rhat']
    return tail_keys('dtail', res, ok.shape[0] * ok.shape[1], n_splits, rhat)


def tail_keys(prefix, res, n_draws, n_splits, rhat):
    """The metrics.json keys of a tail_diagnostics result under ``prefix`` (dtail: the parameters as sampled; fdiag_tail: the
    function-space columns; cdiag_tail: the canonical ordering) with ``rhat``, the rank R-hat of the same columns, and the arrays
    for tail_diagnostics.npz under the same prefix (none for dtail)."""
    from mile_amd import metrics as M
    keys = M.tail_diagnostics_summary(res, n_draws, n_splits, rhat=rhat, prefix=prefix)
    stem = '' if prefix == 'dtail' else prefix[:-len('tail')]
    arrays = {stem + k: res[k].detach().cpu().numpy() for k in M.TAIL_OUTPUTS + ('quantiles',)}
    return keys, arrays


def canonical_refusal(model, activation, sign):
    """Why --canonical-diagnostics cannot run on an experiment of ``model`` with ``activation``, or None."""
    if model != 'FCN':
        return (f'--canonical-diagnostics: the canonical hidden-unit ordering is defined for FCN experiments only; this one is '
                f'{model} (--function-diagnostics compares chains of any model)')
    if sign and activation != 'tanh':
        return (f'--canonical-sign: fixing the signs of the hidden units needs an odd activation (tanh); this net uses '
                f'{activation}, whose units have no sign symmetry to remove')
    return None


def canonical_diagnostic_metrics(samples, spec, n_splits, key, sign, device, tail_splits=None):
    """--canonical-diagnostics: the statistics of --diagnostics on the canonical hidden-unit ordering of the finite chains
    (mile_amd.metrics.canonical_diagnostics: mile_canonicalize_fcn, then mile_chain_diagnostics, on the device), and how often the
    order of each hidden layer changes from one draw to the next.  samples [C, S, d] (host).  Returns the cdiag_* keys of
    metrics.json and the arrays of canonical_diagnostics.npz."""
    from mile_amd.metrics import canonical_diagnostics
    fin = np.isfinite(samples).all(axis=(1, 2))
    ok = np.ascontiguousarray(samples[fin])
    if ok.shape[0] == 0:
        raise SystemExit('--canonical-diagnostics: no chain with finite samples')
    res = canonical_diagnostics(spec, torch.from_numpy(ok).to(device), n_splits, key=key, sign=sign)
    arr = {k: v.detach().cpu().numpy() for k, v in res.items()}
    out = diagnostic_keys('cdiag', arr, spec, n_splits)
    out['cdiag_key'], out['cdiag_sign'] = key, bool(sign)
    for l in range(arr['switches'].shape[1]):
        out[f'cdiag_switch_rate_layer{l}'] = float(np.mean(arr['switches'][:, l] / max(ok.shape[1] - 1, 1)))
    if tail_splits is None:
        return out, arr
    from mile_amd import metrics as M
    canon = M.canonicalize(spec, torch.from_numpy(ok).to(device), key, sign, return_perm=True)[0]
    return out, arr, tail_keys('cdiag_tail', M.tail_diagnostics(canon, tail_splits), ok.shape[0] * ok.shape[1], tail_splits, res['rhat'])


def aligned_refusal(model, activation, sign):
    """Why --aligned-diagnostics cannot run on an experiment of ``model`` with ``activation``, or None."""
    if model != 'FCN':
        return (f'--aligned-diagnostics: the alignment of hidden units to a reference draw is defined for FCN experiments only; '
                f'this one is {model} (--function-diagnostics compares chains of any model)')
    if sign and activation != 'tanh':
        return (f'--align-sign: flipping matched hidden units needs an odd activation (tanh); this net uses {activation}, whose '
                f'units have no sign symmetry to remove')
    return None


def aligned_diagnostic_metrics(samples, spec, n_splits, reference, rounds, sign, device, tail_splits=None):
    """--aligned-diagnostics: the statistics of --diagnostics on the finite chains with every draw's hidden units matched to those
    of one reference draw by assignment (mile_amd.metrics.aligned_diagnostics: mile_align_fcn, then mile_chain_diagnostics, on the
    device), how often each chain's matching of a layer changes from one draw to the next, and the matched similarity per layer.
    samples [C, S, d] (host); reference 'first' or a row of d floats.  Returns the adiag_* keys of metrics.json and the arrays of
    aligned_diagnostics.npz."""
    from mile_amd import metrics as M
    fin = np.isfinite(samples).all(axis=(1, 2))
    ok = np.ascontiguousarray(samples[fin])
    if ok.shape[0] == 0:
        raise SystemExit('--aligned-diagnostics: no chain with finite samples')
    ref = reference if isinstance(reference, str) else torch.from_numpy(np.ascontiguousarray(reference, dtype=np.float32)).to(device)
    res = M.aligned_diagnostics(spec, torch.from_numpy(ok).to(device), n_splits, reference=ref, rounds=rounds, sign=sign)
    aligned, dropped = res.pop('theta'), res.pop('dropped')
    arr = {k: v.detach().cpu().numpy() for k, v in res.items()}
    out = diagnostic_keys('adiag', arr, spec, n_splits)
    out['adiag_reference'] = reference if isinstance(reference, str) else 'file'
    out['adiag_rounds'], out['adiag_sign'], out['adiag_dropped'] = int(rounds), bool(sign), int(dropped)
    for l in range(arr['switches'].shape[1]):
        out[f'adiag_switch_rate_layer{l}'] = float(np.mean(arr['switches'][:, l] / max(ok.shape[1] - 1, 1)))
        out[f'adiag_score_mean_layer{l}'] = float(arr['score_mean'][l])
    if tail_splits is None:
        return out, arr
    return out, arr, tail_keys('adiag_tail', M.tail_diagnostics(aligned, tail_splits), ok.shape[0] * ok.shape[1], tail_splits, res['rhat'])


def function_diagnostic_metrics(eng, samples, x, y, task, n_splits, tail_splits=None):
    """--function-diagnostics: ESS, split R-hat and within / between chain variance of what the finite chains PREDICT on the
    split's rows (mile_amd.metrics.function_diagnostics: mile_function_diagnostics on the device).  samples [C, S, d] (host).
    Returns the fdiag_* keys of metrics.json and the arrays of function_diagnostics.npz."""
    from mile_amd import metrics as M
    fin = np.isfinite(samples).all(axis=(1, 2))
    ok = np.ascontiguousarray(samples[fin])
    if ok.shape[0] == 0:
        raise SystemExit('--function-diagnostics: no chain with finite samples')
    res = M.function_diagnostics(eng, torch.from_numpy(ok), torch.from_numpy(x), torch.from_numpy(y), n_splits=n_splits,
                                 return_columns=tail_splits is not None)
    out = {'fdiag_n_splits': int(n_splits), 'fdiag_chain_ids': [int(c) for c in np.nonzero(fin)[0]]}
    out.update(M.function_diagnostics_summary(res, int(x.shape[0]), int(res['Q']), task))
    arrays = {k: res[k].detach().cpu().numpy() for k in ('wcv', 'bcv', 'rhat', 'ess', 'crhat', 'loglik_sum', 'chain_summary')}
    arrays['Q'] = np.int64(res['Q'])
    if tail_splits is None:
        return out, arrays
    tail = M.tail_diagnostics(res['columns'], tail_splits, plane=True)                # every column, the summed log-likelihood's too
    return out, arrays, tail_keys('fdiag_tail', tail, ok.shape[0] * ok.shape[1], tail_splits, res['rhat'])


def moment_metrics(moments, dropped, y, task):
    """--moments: the metrics.json keys and the moments.npz arrays of posterior-predictive moments [N, W]
    (Engine.predict_moments, or metrics.predictive_moments of raw outputs), ``dropped`` [N] and the split's targets ``y``.
    Keys: the mean over the rows of each column (rows without a finite draw left out), the draws dropped in all, and for
    regression the RMSE of the mean prediction."""
    from mile_amd import metrics as M
    mom = moments.detach().double().cpu()
    drop = dropped.detach().cpu().numpy().astype(np.int32)
    col = [float(v) for v in torch.nanmean(mom, dim=0)]
    if task == 'regr':
        names = ['mean', 'epistemic_var', 'aleatoric_var']
        arrays = {n: mom[:, i].numpy().astype(np.float32) for i, n in enumerate(names)}
        out = {f'moments_{n}': col[i] for i, n in enumerate(names)}
        fin = torch.isfinite(mom[:, 0])
        yt = torch.as_tensor(np.ascontiguousarray(y), dtype=torch.float64).reshape(-1)
        out['moments_rmse'] = float(M.rmse_from_moments(yt[fin], mom[fin])) if bool(fin.any()) else float('nan')
    else:
        K = mom.shape[1] - 2
        arrays = {'probs': mom[:, :K].numpy().astype(np.float32), 'entropy': mom[:, K].numpy().astype(np.float32),
                  'mutual_information': mom[:, K + 1].numpy().astype(np.float32)}
        out = {'moments_probs': col[:K], 'moments_entropy': col[K], 'moments_mutual_information': col[K + 1]}
    arrays['dropped'] = drop
    out['moments_dropped'] = int(drop.sum())
    return out, arrays


def sensitivity_refusal(model: str):
    """Why --sensitivities cannot run on this experiment, or None."""
    if model != 'FCN':
        return (f'--sensitivities: input sensitivities are for FCN (tabular) experiments; this one is {model}, whose inputs are '
                'token ids or image pixels')
    return None


def partial_dependence_refusal(model: str):
    """Why --partial-dependence cannot run on this experiment, or None."""
    if model != 'FCN':
        return (f'--partial-dependence: partial dependence is for FCN (tabular) experiments; this one is {model}, whose inputs are '
                'token ids or image pixels')
    return None


def partial_dependence_metrics(res, grid, features, feature_names=None):
    """--partial-dependence: the metrics.json keys and the partial_dependence.npz arrays of Engine.predict_partial_dependence's
    result ``res`` (or metrics.partial_dependence_dense's) on ``grid`` [Fs, G] of the selected ``features``.  Keys, each [Fs][P]
    per selected feature and head output, in the network's units (metrics.partial_dependence_summary): ``pd_importance`` the sd
    of the partial dependence over the grid, ``pd_span``, ``pd_slope``, ``pd_band`` the mean width of the posterior band,
    ``pd_chain_sd`` and ``pd_chain_ratio`` the chains' disagreement on the curve, alone and against the band,
    ``pd_ice_heterogeneity`` the spread of the centred ICE curves over the rows; ``pd_features``, ``pd_grid_points``,
    ``pd_dropped`` the (draw, row, feature) triples left out.  Arrays: the grid, the eight outputs, ``feature_index`` and, with
    names, ``feature_names`` of the selected features."""
    from mile_amd import metrics as M
    summ = M.partial_dependence_summary(res, grid)
    out = {f'pd_{k}': summ[k] for k in ('importance', 'span', 'slope', 'band', 'chain_sd', 'chain_ratio', 'ice_heterogeneity')}
    out.update(pd_features=[int(f) for f in features], pd_grid_points=int(grid.shape[1]), pd_dropped=int(res['dropped'].sum()))
    arrays = {k: res[k].detach().cpu().numpy() for k in M.PD_OUTPUTS}
    arrays['grid'] = grid.detach().cpu().numpy()
    arrays['feature_index'] = np.asarray([int(f) for f in features], dtype=np.int64)
    if feature_names is not None:
        arrays['feature_names'] = np.asarray([feature_names[int(f)] for f in features])
        out['pd_feature_names'] = [str(feature_names[int(f)]) for f in features]
    return out, arrays


def feature_labels(features, F: int):
    """The data config's column names where it gives exactly one per input, else None."""
    if isinstance(features, (list, tuple)) and len(features) == F:
        return [str(f) for f in features]
    return None


def sensitivity_metrics(res, feature_names=None):
    """--sensitivities: the metrics.json keys and the sensitivities.npz arrays of Engine.predict_sensitivities' result ``res``
    (or metrics.sensitivities_dense's).  Keys, each [P][F] per head output and feature, in the network's units (normalised inputs
    and targets): ``sens_ape`` the ensemble's average partial effect, ``sens_importance`` the mean |effect|, ``sens_chain_sd``
    the disagreement of the chains' average effects, ``sens_decided`` the share of rows whose sign is decided, ``sens_ranking``
    the features by falling importance (``sens_ranked_names`` with names), ``sens_dropped`` the (draw, row) pairs left out.
    Arrays: the seven outputs, and ``feature_names`` or ``feature_index``."""
    from mile_amd import metrics as M
    summ = M.sensitivity_summary(res, feature_names)
    out = {'sens_ape': summ['ape'], 'sens_importance': summ['importance'], 'sens_chain_sd': summ['chain_sd'],
           'sens_decided': summ['decided'], 'sens_ranking': summ['ranking'], 'sens_dropped': int(res['dropped'].sum())}
    if feature_names is not None:
        out['sens_ranked_names'] = summ['ranked_names']
    arrays = {k: res[k].detach().cpu().numpy() for k in M.SENS_OUTPUTS}
    F = arrays['mean'].shape[2]
    if feature_names is not None:
        arrays['feature_names'] = np.asarray(feature_names)
    else:
        arrays['feature_index'] = np.arange(F, dtype=np.int64)
    return out, arrays


def running_metrics(res):
    """--running: the metrics.json keys and the running_lppd.npz arrays of Engine.lppd_stream's result ``res``.  Keys: the
    ensemble LPPD and each chain's from the stream, the first and last value of both curves (``running_lppd``, the LPPD of all draws, is
    also the last point of the ensemble curve), and the (draw, row) pairs dropped in all."""
    arrays = {k: res[k].detach().cpu().numpy() for k in ('curve_points', 'run_chain', 'run_ens', 'chain_lppd', 'row_lppd', 'dropped')}
    pc = [float(v) for v in arrays['chain_lppd']]
    out = {'running_points': int(len(arrays['curve_points'])), 'running_lppd': float(res['lppd'].item()),
           'running_per_chain_lppd': pc, 'running_per_chain_lppd_median': float(np.nanmedian(pc)),
           'running_ens_first': float(arrays['run_ens'][0]), 'running_ens_last': float(arrays['run_ens'][-1]),
           'running_chain_first': float(arrays['run_chain'][0]), 'running_chain_last': float(arrays['run_chain'][-1]),
           'running_dropped': int(arrays['dropped'].sum())}
    return out, arrays


def interval_metrics(quant, pit, dropped, levels, coverages):
    """--intervals: the metrics.json keys and the intervals.npz arrays of the ensemble's exact predictive quantiles [N, Q] at
    ``levels`` (``metrics.interval_levels(coverages)``), the PIT [N] and ``dropped`` [N] (Engine.predict_quantiles, or
    metrics.mixture_quantiles / mixture_pit of raw outputs).  Keys: the observed coverage of each central interval from the
    PIT (no draws, no seed), the calibration error of those, the mean width of each interval, the draws dropped in all."""
    from mile_amd import metrics as M
    q = quant.detach().double().cpu()
    lv = [float(v) for v in levels]
    cov = M.coverage_from_pit(pit.detach().cpu(), coverages)
    out = {}
    for c, v in zip(coverages, cov):
        lo, hi = (lv.index(float(a)) for a in M.get_quantiles(float(c)))
        out[f'intervals_coverage_{c}'] = float(v)
        out[f'intervals_width_{c}'] = float(torch.nanmean(q[:, hi] - q[:, lo]))
    out['intervals_cal_error'] = float(M.calibration_error(coverages, cov).item())
    drop = dropped.detach().cpu().numpy().astype(np.int32)
    out['intervals_dropped'] = int(drop.sum())
    arrays = {'levels': np.asarray(lv, dtype=np.float64), 'quantiles': q.numpy().astype(np.float32),
              'pit': pit.detach().cpu().numpy().astype(np.float32), 'dropped': drop}
    return out, arrays


def loo_metrics(rows):
    """--loo: the metrics.json keys and the loo.npz arrays of the per-row PSIS-LOO / WAIC result ``rows`` (Engine.loo_stream, or
    metrics.psis_loo of a pointwise tensor) on the train split.  Keys: ``loo_`` + every total of ``metrics.loo_summary``, the
    rows evaluated and the draws dropped in all."""
    from mile_amd.metrics import loo_summary
    arrays = {k: rows[k].detach().cpu().numpy() for k in ('lppd', 'p_waic', 'elpd_loo', 'khat', 'dropped')}
    out = {f'loo_{k}': v for k, v in loo_summary(arrays).items()}
    out['loo_n_points'] = int(arrays['lppd'].shape[0])
    out['loo_dropped'] = int(arrays['dropped'].sum())
    return out, arrays


def loo_predict_metrics(rows, y, task, coverages):
    """--loo-predict: the metrics.json keys and the loo_predict.npz arrays of the per-row leave-one-out predictions ``rows``
    (metrics.loo_predict) on the train split.  Keys: ``loopred_`` + every entry of ``metrics.loo_predict_summary``.  Arrays:
    expect, posterior, ess_w, khat, dropped per row and, for regression, pit (column 3 of expect, whose sum of weights is 1 only up
    to rounding, clipped to [0, 1])."""
    from mile_amd.metrics import loo_predict_summary
    out = {f'loopred_{k}': v for k, v in loo_predict_summary(rows, y, task, coverages).items()}
    arrays = {k: rows[k].detach().cpu().numpy() for k in ('expect', 'posterior', 'ess_w', 'khat', 'dropped')}
    if task == 'regr':
        arrays['pit'] = np.clip(arrays['expect'][:, 3], 0.0, 1.0)
    return out, arrays


def stacking_refusal(n_chains, n_draws):
    """Why --stacking cannot run on ``n_chains`` chains of ``n_draws`` draws, or None."""
    if n_draws < 2:
        return f'--stacking: PSIS-LOO of a chain needs at least 2 draws per chain; this experiment kept {n_draws}'
    if n_chains > 1024:
        return f'--stacking: at most 1024 chains (mile_chain_loo_stream, mile_stack_eval); this experiment has {n_chains}'
    return None


def stacking_metrics(train_rows, lpd_eval, eval=None):
    """--stacking: the metrics.json keys and the stacking.npz arrays from the per-chain PSIS-LOO of the train split
    ``train_rows`` (Engine.chain_loo_stream: ``elpd_loo`` and ``khat`` [C, N_train]) and the per-chain log predictive density of
    the evaluated split ``lpd_eval`` [C, N].  The weights maximise the leave-one-out log score of the weighted mixture of the
    chains (``metrics.stacking_weights``; ``eval``: Engine.stack_eval, None for the torch form); ``stacking_lppd`` is the
    weighted LPPD of the evaluated split, ``stacking_lppd_equal`` the same at 1 / C -- the ensemble's LPPD -- and
    ``stacking_gain`` their difference."""
    from mile_amd import metrics as M
    sol = M.stacking_weights(train_rows['elpd_loo'], eval=eval)
    w = sol['w']
    summary = M.stacking_summary(train_rows)
    C_ = int(w.shape[0])
    weighted = M.weighted_lppd(lpd_eval, w, eval=eval)
    equal = M.weighted_lppd(lpd_eval, np.full(C_, 1.0 / C_), eval=eval)
    out = {'stacking_lppd': weighted, 'stacking_lppd_equal': equal, 'stacking_gain': weighted - equal,
           'stacking_gap': float(sol['gap']), 'stacking_iterations': int(sol['iterations']),
           'stacking_converged': bool(sol['converged']), 'stacking_effective_chains': float(1.0 / np.sum(w * w)),
           'stacking_khat_bad': int(sum(summary['chain_khat_bad'])), 'stacking_weights': [float(v) for v in w]}
    arrays = {'weights': np.asarray(w, dtype=np.float64), 'chain_elpd_loo': np.asarray(summary['chain_elpd_loo'], dtype=np.float64),
              'chain_khat_bad': np.asarray(summary['chain_khat_bad'], dtype=np.int64), 'gap': np.float64(sol['gap']),
              'n_train': np.int64(summary['n_rows']), 'n_train_used': np.int64(sol['used']), 'n_eval': np.int64(lpd_eval.shape[1])}
    return out, arrays


CRPS_GRAM_BYTES = 256 << 20             # --crps asks for the Gram matrices [N, C, C] fp64 only while they fit


def stacked_weights(w):
    """The solved stacking weights as the weighted entry points take them: clipped at 0 and renormalised, float64 [C]."""
    w = np.clip(np.asarray(w, dtype=np.float64), 0.0, None)
    return w / w.sum()


def stacked_interval_metrics(quant, pit, levels, coverages):
    """--stacking with --intervals: ``interval_metrics`` of the stacking-weighted mixture (Engine.predict_quantiles_weighted),
    the keys as ``intervals_stacked_*`` and the arrays as ``quantiles_stacked``, ``pit_stacked``."""
    keys, arrays = interval_metrics(quant, pit, torch.zeros(1, dtype=torch.int32), levels, coverages)
    out = {k.replace('intervals_', 'intervals_stacked_', 1): v for k, v in keys.items() if k != 'intervals_dropped'}
    return out, {'quantiles_stacked': arrays['quantiles'], 'pit_stacked': arrays['pit']}


def stacked_calibration_metrics(res, w, y, n_bins):
    """--stacking with --calibration: NLL, Brier score, ECE and accuracy of P = sum_c w_c P_c, from the calibration result's
    per-chain probabilities through ``metrics.weighted_class_probs`` and ``metrics.calibration_decide``."""
    from mile_amd import metrics as M
    P, kept = M.weighted_class_probs(res['probs'][:-1].double(), res['kept'][:-1], w)
    dec = M.calibration_decide(P[None], kept[None], torch.as_tensor(y), res['coverages'], n_bins)
    s = M.calibration_summary({'totals': dec['totals'], 'bins': dec['bins'], 'coverages': res['coverages']})[0]
    return {'calibration_stacked_nll': s['nll'], 'calibration_stacked_brier': s['brier'], 'calibration_stacked_ece': s['ece'],
            'calibration_stacked_accuracy': s['acc']}


def crps_refusal(task, n_chains):
    """Why --crps cannot run on this experiment, or None."""
    if task != 'regr':
        return ('--crps: the CRPS scores a predictive density on the real line, so it is for regression experiments; this one is '
                'classification (--calibration is its counterpart)')
    if n_chains > 1024:
        return f'--crps: at most 1024 chains (mile_crps_stream); this experiment has {n_chains}'
    return None


def crps_outputs(n_rows, n_chains):
    """The outputs --crps asks Engine.crps_stream for: ``gram`` only while N * C^2 * 8 B <= 256 MiB."""
    base = ('crps_chain', 'spread_chain', 'crps_mix', 'spread_mix', 'dropped')
    return base + (('gram',) if n_rows * n_chains * n_chains * 8 <= CRPS_GRAM_BYTES else ())


def crps_metrics(rows, stride, stacked=None):
    """--crps: the metrics.json keys and the crps.npz arrays of Engine.crps_stream's result ``rows`` (or
    metrics.mixture_crps_dense's).  The call's weight vectors are 1 / C and, with ``stacked`` [C] (the weights of --stacking),
    those: ``crps`` / ``crps_spread`` (the pooled ensemble of all kept draws), ``crps_uniform``, ``crps_stacked`` with their
    standard errors over rows, what pooling gains over the chains one by one, each chain's own CRPS and spread with the
    median, the largest row-mean energy distance between two chains (with ``gram``), the thinning stride and the draws dropped."""
    from mile_amd.metrics import crps_summary
    C_ = int(rows['crps_chain'].shape[0])
    W = [np.full(C_, 1.0 / C_)] + ([np.asarray(stacked, dtype=np.float64)] if stacked is not None else [])
    arrays = {k: v.detach().cpu().numpy() for k, v in rows.items()}
    s = crps_summary(arrays, weights=np.stack(W))
    out = {'crps': s['crps'], 'crps_se': s['crps_se'], 'crps_spread': s['spread'], 'crps_spread_se': s['spread_se'],
           'crps_uniform': s['mix_crps'][0], 'crps_uniform_se': s['mix_crps_se'][0], 'crps_uniform_pooling_gain': s['mix_pooling_gain'][0],
           'crps_per_chain': s['chain_crps'], 'crps_per_chain_median': float(np.nanmedian(s['chain_crps'])),
           'crps_per_chain_spread': s['chain_spread'], 'crps_rows_nan': s['rows_nan'], 'crps_thin_stride': int(stride),
           'crps_dropped': int(arrays['dropped'].sum())}
    if stacked is not None:
        out.update({'crps_stacked': s['mix_crps'][1], 'crps_stacked_se': s['mix_crps_se'][1],
                    'crps_stacked_pooling_gain': s['mix_pooling_gain'][1]})
    if 'energy_distance' in s:
        out['crps_energy_distance_max'] = float(np.max(s['energy_distance']))
        arrays['energy_distance'] = np.asarray(s['energy_distance'], dtype=np.float64)
    arrays['weights'] = np.stack(W)
    arrays['thin_stride'] = np.int64(stride)
    return out, arrays


def calibration_metrics(res, n_bins):
    """--calibration: the metrics.json keys and the calibration.npz arrays of a calibration result ``res``
    (Engine.calibration_stream, or metrics.classification_calibration of logits).  Keys: ``calibration_`` + every entry of the
    ensemble's ``metrics.calibration_summary``, the per-chain ACC, Brier score, NLL and ECE with their medians, the bins used
    and the (draw, row) pairs dropped in all."""
    from mile_amd.metrics import calibration_summary
    arrays = {k: res[k].detach().cpu().numpy() for k in ('coverages', 'order', 'set_size', 'rank', 'kept', 'bins', 'totals')}
    arrays['probs'] = res['probs'][-1].detach().cpu().numpy().astype(np.float32)
    summary = calibration_summary(arrays)
    out = {f'calibration_{k}': v for k, v in summary[-1].items()}
    for k in ('acc', 'brier', 'nll', 'ece'):
        pc = [s[k] for s in summary[:-1]]
        out[f'calibration_per_chain_{k}'] = pc
        out[f'calibration_per_chain_{k}_median'] = float(np.nanmedian(pc))
    out['calibration_n_bins'] = int(n_bins)
    return out, arrays


def build_parser():
    ap = argparse.ArgumentParser(description='LPPD / NLL of the samples of an experiment directory')
    ap.add_argument('--diagnostics', type=int, nargs='?', const=2, default=None, metavar='N_SPLITS',
                    help='per-parameter chain diagnostics of ALL parameters (ESS, split R-hat with N_SPLITS splits, default 2, '
                         'within / between chain variance): diag_* keys in metrics.json and the arrays in diagnostics.npz; the HIP '
                         'kernels take 4 <= n_samples <= 4096, other lengths run in plain torch')
    ap.add_argument('--function-diagnostics', type=int, nargs='?', const=2, default=None, metavar='N_SPLITS',
                    help='chain diagnostics in FUNCTION space, streamed on the device (mile_function_diagnostics): ESS, split R-hat '
                         'with N_SPLITS splits (default 2) and within / between chain variance of every prediction on the rows of '
                         '--split (regression: mu, log sigma and the log-likelihood of each row; classification: the class '
                         'probabilities and the log-likelihood) and of the summed log-likelihood of each draw, over the finite '
                         'chains.  Chains in permuted copies of one mode agree here although their parameters do not.  The kernels '
                         'take 4 <= n_samples <= 4096 with N_SPLITS dividing n_samples into pieces of at least 2 draws; other '
                         'lengths are refused with the library\'s message (no torch fall-back, unlike --diagnostics).  fdiag_* keys '
                         'in metrics.json (fdiag_rhat_max, fdiag_ess_min, fdiag_r_eff_mean, per-quantity and per-chain figures) and '
                         'wcv, bcv, rhat, ess, crhat, loglik_sum, chain_summary, Q in function_diagnostics.npz')
    ap.add_argument('--canonical-diagnostics', type=int, nargs='?', const=2, default=None, metavar='N_SPLITS',
                    help='FCN experiments: the statistics of --diagnostics on the CANONICAL hidden-unit ordering of every draw of '
                         'the finite chains (mile_canonicalize_fcn, then mile_chain_diagnostics, on the device): the units of each '
                         'hidden layer sorted by --canonical-key, which removes the permutation symmetry that makes chains in '
                         'permuted copies of one mode fail every per-parameter check.  cdiag_* keys in metrics.json mirror the '
                         'diag_* keys, plus cdiag_key, cdiag_sign and cdiag_switch_rate_layer<l> (the share of draws whose order of '
                         'hidden layer l differs from the draw before: ordering by a key gives order statistics, not an alignment to '
                         'a reference mode, and a high rate says the key does not separate the units of this posterior); wcv, bcv, '
                         'rhat, ess, crhat, switches in canonical_diagnostics.npz.  No ReLU rescaling, no sigmoid reflection; hidden '
                         'widths above 1024 run in plain torch')
    ap.add_argument('--tail-diagnostics', type=int, nargs='?', const=2, default=None, metavar='N_SPLITS',
                    help='tail diagnostics of ALL parameters of the finite chains on the device (mile_chain_diagnostics_tail): the '
                         'POOLED multi-chain ESS of the rank-normalised draws (bulk), of the 5 %% / 95 %% tails and of the mean, the '
                         'Monte Carlo standard error of the posterior mean, and the split R-hat of the draws folded about their median, '
                         'which sees chains that agree in location and differ in scale.  dtail_* keys in metrics.json (ess_bulk and '
                         'ess_tail min / median, rhat_folded median / max, rhat_rank_max = max over the parameters of max(rhat, '
                         'rhat_folded), mcse_mean_over_sd_max, ess_bulk_share) and ess_bulk, ess_tail, ess_mean, mcse_mean, '
                         'rhat_folded, quantiles in tail_diagnostics.npz.  With --function-diagnostics also fdiag_tail_* (every '
                         'function-space column, fdiag_* arrays in the npz), with --canonical-diagnostics also cdiag_tail_*')
    ap.add_argument('--canonical-key', choices=['bias', 'norm'], default='bias',
                    help='--canonical-diagnostics orders the hidden units by their bias (default) or by the squared norm of their '
                         'bias and incoming weights')
    ap.add_argument('--canonical-sign', action='store_true',
                    help='--canonical-diagnostics on a tanh net: flip every hidden unit whose bias is negative first (the sign '
                         'symmetry of an odd activation)')
    ap.add_argument('--aligned-diagnostics', type=int, nargs='?', const=2, default=None, metavar='N_SPLITS',
                    help='FCN experiments: the statistics of --diagnostics on the draws of the finite chains ALIGNED to one reference '
                         'draw (mile_align_fcn, then mile_chain_diagnostics, on the device): per hidden layer, in a forward sweep, the '
                         'units of every draw are matched to the reference\'s by a linear assignment problem on the similarity of their '
                         'bias and incoming weights (the last hidden layer also of its outgoing weights), so that a parameter is the same '
                         'unit in every draw and chain -- an alignment to a mode, where --canonical-diagnostics gives order statistics.  '
                         'adiag_* keys in metrics.json mirror the diag_* keys, plus adiag_reference, adiag_rounds, adiag_sign, '
                         'adiag_dropped (draws with a non-finite similarity, copied unchanged), adiag_switch_rate_layer<l> (the share of '
                         'draws whose matching of hidden layer l differs from the draw before; 0 where each chain stays in one copy of '
                         'the mode) and adiag_score_mean_layer<l>; wcv, bcv, rhat, ess, crhat, switches (per chain and layer), scores, '
                         'score_mean and reference in aligned_diagnostics.npz; with --tail-diagnostics also adiag_tail_*.  Hidden widths '
                         'above 128 run in scipy on the host.  No ReLU rescaling, no sigmoid reflection')
    ap.add_argument('--align-reference', default='first', metavar='first|PATH.npy',
                    help='--aligned-diagnostics aligns to the first draw of the first finite chain (default) or to the row of d floats '
                         'in PATH.npy')
    ap.add_argument('--align-rounds', type=int, default=2, metavar='R',
                    help='--aligned-diagnostics: rounds of alignment (default 2); from the second on the reference is the mean of the '
                         'draws as the round before aligned them')
    ap.add_argument('--align-sign', action='store_true',
                    help='--aligned-diagnostics on a tanh net: also flip a matched unit whose similarity to its reference unit is '
                         'negative (the sign symmetry of an odd activation)')
    ap.add_argument('--moments', action='store_true',
                    help='posterior-predictive moments of all draws on the split, reduced on the device (mile_predict_moments): '
                         'moments_* keys in metrics.json and the per-row arrays in moments.npz (regression: mean, epistemic_var, '
                         'aleatoric_var; classification: probs, entropy, mutual_information; both: dropped)')
    ap.add_argument('--running', type=int, nargs='?', const=64, default=None, metavar='N_POINTS',
                    help='LPPD against the number of draws, streamed on the device (mile_lppd_stream) at N_POINTS draw counts spaced '
                         'geometrically from 1 to n_samples (default 64): running_* keys in metrics.json -- the ensemble and per-chain '
                         'LPPD from the stream, the ends of both curves -- and curve_points, run_chain, run_ens, chain_lppd, row_lppd, '
                         'dropped in running_lppd.npz')
    ap.add_argument('--intervals', action='store_true',
                    help='regression: exact quantiles of the ensemble\'s predictive mixture at the levels of --coverages and the PIT, '
                         'solved on the device (mile_predict_quantiles): intervals_coverage_<c>, intervals_width_<c>, '
                         'intervals_cal_error and intervals_dropped in metrics.json -- no draws, so no seed and no Monte-Carlo noise -- '
                         'and levels, quantiles, pit, dropped in intervals.npz')
    ap.add_argument('--loo', action='store_true',
                    help='PSIS-LOO and WAIC of the ensemble, streamed on the device (mile_loo_stream).  Always on the TRAIN split, '
                         'whatever --split says: leave-one-out estimates out-of-sample fit from the rows the sampler conditioned on, '
                         'and means nothing on held-out rows.  loo_* keys in metrics.json (elpd_loo, p_loo, elpd_waic, p_waic with '
                         'standard errors, lppd_sum, the counts of rows with khat > 0.7, without a tail fit and with p_waic > 0.4) and '
                         'lppd, p_waic, elpd_loo, khat, dropped per row in loo.npz')
    ap.add_argument('--loo-predict', action='store_true',
                    help='leave-one-out predictions of the ensemble from the PSIS weights of --loo, streamed on the device '
                         '(mile_loo_predict_stream).  Always on the TRAIN split, like --loo; --loo-r-eff and --coverages apply.  '
                         'loopred_* keys in metrics.json -- regression: rmse, r2, var_epistemic, var_aleatoric, coverage_<c> and '
                         'cal_error from the LOO-PIT; classification: accuracy, brier, nll (= -mean elpd_loo), ece, mce; each again as '
                         '*_insample from the posterior that has seen every row; the share of rows with khat > 0.7 and the minimum and '
                         'median importance-sampling ESS -- and expect, posterior, ess_w, khat, dropped (regression: pit) per row in '
                         'loo_predict.npz')
    ap.add_argument('--calibration', type=int, nargs='?', const=15, default=None, metavar='N_BINS',
                    help='classification: prediction sets and calibration of every chain and of the ensemble, streamed on the device '
                         '(mile_calibration_stream) -- highest-probability sets at the levels of --coverages, the rank of the label, Brier '
                         'score, NLL, accuracy and N_BINS equal-width reliability bins (default 15): calibration_* keys in metrics.json '
                         '(acc, brier, nll, ece, mce, coverage_<c>, set_size_<c>, cal_error of the ensemble, per-chain lists and medians, '
                         'calibration_dropped) and coverages, probs, order, set_size, rank, kept, bins, totals in calibration.npz -- no '
                         'draws, so no seed')
    ap.add_argument('--stacking', action='store_true',
                    help='stacking weights of the chains (Yao et al. 2018), for chains that do not mix: PSIS-LOO of every chain on '
                         'its own on the TRAIN split (mile_chain_loo_stream), the simplex weights that maximise the leave-one-out log '
                         'score of the weighted mixture (mile_stack_eval behind a Newton / active-set solver), and what they buy on '
                         '--split: stacking_lppd (weighted), stacking_lppd_equal (1 / C: the lppd above), stacking_gain, stacking_gap '
                         '(a certified bound on the score left on the table), stacking_iterations, stacking_converged, '
                         'stacking_effective_chains (1 / sum w^2), stacking_khat_bad (chain rows with khat > 0.7) and stacking_weights in '
                         'metrics.json; weights, chain_elpd_loo, chain_khat_bad, gap, n_train, n_train_used, n_eval in stacking.npz.  '
                         'Needs at least 2 draws per chain; --loo-r-eff applies.  Next to --intervals, --moments or --calibration the '
                         'stacked mixture is reported beside the ensemble: intervals_stacked_coverage_<c>, intervals_stacked_width_<c>, '
                         'intervals_stacked_cal_error (quantiles_stacked and pit_stacked in intervals.npz; mile_predict_quantiles_weighted), '
                         'moments_stacked_rmse, calibration_stacked_nll, _brier, _ece and _accuracy')
    ap.add_argument('--crps', action='store_true',
                    help='regression: the exact CRPS of the predictive mixture on --split, from all pairs of draws on the device '
                         '(mile_crps_stream; closed form, so no draws and no seed): crps (the pooled ensemble), crps_spread, '
                         'crps_uniform (chains weighted 1 / C), each with _se over rows, crps_uniform_pooling_gain, crps_per_chain, '
                         'crps_per_chain_median, crps_per_chain_spread, crps_energy_distance_max, crps_rows_nan, crps_thin_stride and '
                         'crps_dropped in metrics.json; the per-row arrays crps_chain, spread_chain, crps_mix, spread_mix, dropped, '
                         'weights, thin_stride (and gram, energy_distance while N C^2 8 B <= 256 MiB) in crps.npz.  With --stacking in '
                         'the same call the stacked weights are scored too: crps_stacked, crps_stacked_se, crps_stacked_pooling_gain')
    ap.add_argument('--crps-max-draws', type=int, default=131072, metavar='M',
                    help='--crps thins every chain to its draws j = 0 mod k, k = ceil(n_chains * n_samples / M), so that about M '
                         'draws enter the pair sums (default 131072; k is recorded as crps_thin_stride)')
    ap.add_argument('--loo-r-eff', '--r-eff', type=float, default=1.0, metavar='R_EFF',
                    help='relative efficiency of the draws behind the PSIS tail length of --loo and --stacking (default 1: independent draws)')
    ap.add_argument('--sensitivities', action='store_true',
                    help='FCN experiments: input sensitivities of the ensemble on the split, reduced on the device '
                         '(mile_predict_sensitivities): per head output and feature the average partial effect, the importance, the '
                         'chains\' disagreement and the share of rows with a decided sign as sens_* keys in metrics.json, and the '
                         'per-row and per-chain arrays in sensitivities.npz.  In the network\'s units: normalised inputs and targets')
    ap.add_argument('--partial-dependence', type=int, nargs='?', const=20, default=None, metavar='G',
                    help='FCN experiments: partial dependence and ICE curves of the ensemble on the split, reduced on the device '
                         '(mile_predict_partial_dependence), every selected feature over G grid values (default 20) at the 5 %% - 95 %% '
                         'quantiles of its own column: per feature and head output the importance, span, posterior band, chains\' '
                         'disagreement and ICE heterogeneity as pd_* keys in metrics.json, and the grid and every output in '
                         'partial_dependence.npz.  In the network\'s units: normalised inputs and targets')
    ap.add_argument('--pd-features', type=int, nargs='+', default=None, metavar='I',
                    help='the features of --partial-dependence, as distinct column indices (default: all); refused without that option')
    ap.add_argument('--exp', '-e', required=True, help='experiment directory (holds config.yaml and samples/)')
    ap.add_argument('--split', default='test', choices=['train', 'valid', 'test'])
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--ess-params', type=int, default=256, help='size of the random parameter subset ESS is evaluated on')
    ap.add_argument('--drop-nonfinite', action='store_true',
                    help='leave out chains with non-finite samples (the reference would report NaN; default: keep them)')
    ap.add_argument('--seed', type=int, default=42, help='seed of the posterior-predictive draws behind ACC / coverage')
    ap.add_argument('--coverages', type=float, nargs='+', default=[0.5, 0.75, 0.9, 0.95],
                    help='nominal coverage levels of the central credible intervals (regression)')
    return ap


def main():
    args = build_parser().parse_args()
    exp = Path(args.exp)
    from mile_amd.callbacks import load_samples_from_dir
    from mile_amd.config import Config
    from mile_amd.metrics import lppd, running_lppd
    from mile_amd.trainer import BDETrainer
    cfg = Config.from_file(exp / 'config.yaml').replace(logging=False)
    tr = BDETrainer.__new__(BDETrainer)            # data + model spec only: no new experiment directory
    if args.intervals and cfg.data.task != 'regr':
        raise SystemExit('--intervals: predictive intervals are for regression experiments; this one is classification')
    if args.calibration is not None and cfg.data.task == 'regr':
        raise SystemExit('--calibration: prediction sets and reliability bins are for classification experiments; this one is '
                         'regression (--intervals is its counterpart)')
    if args.crps and crps_refusal(cfg.data.task, 1):
        raise SystemExit(crps_refusal(cfg.data.task, 1))
    if args.crps and args.crps_max_draws < 1:
        raise SystemExit('--crps-max-draws: at least 1')
    why = canonical_refusal(cfg.model.model, getattr(cfg.model, 'activation', None), args.canonical_sign)
    if args.canonical_diagnostics is not None and why:
        raise SystemExit(why)
    why = aligned_refusal(cfg.model.model, getattr(cfg.model, 'activation', None), args.align_sign)
    if args.aligned_diagnostics is not None and why:
        raise SystemExit(why)
    if args.aligned_diagnostics is not None and args.align_rounds < 1:
        raise SystemExit('--align-rounds: at least 1')
    if args.sensitivities and sensitivity_refusal(cfg.model.model):
        raise SystemExit(sensitivity_refusal(cfg.model.model))
    if args.partial_dependence is not None and partial_dependence_refusal(cfg.model.model):
        raise SystemExit(partial_dependence_refusal(cfg.model.model))
    if args.pd_features is not None and args.partial_dependence is None:
        raise SystemExit('--pd-features selects the features of --partial-dependence: give that option too')
    if args.partial_dependence is not None and not 1 <= args.partial_dependence <= 256:
        raise SystemExit('--partial-dependence: G must be in 1 .. 256')
    align_reference = args.align_reference
    if args.aligned_diagnostics is not None and align_reference != 'first':
        if not Path(align_reference).is_file():
            raise SystemExit(f'--align-reference: {align_reference} is neither "first" nor a .npy file')
        align_reference = np.load(align_reference).reshape(-1)
    tr.build_model(cfg)
    spec = tr.prob_model.spec
    if args.aligned_diagnostics is not None and not isinstance(align_reference, str) and align_reference.shape[0] != spec.n_params:
        raise SystemExit(f'--align-reference: the file holds {align_reference.shape[0]} floats, the net has {spec.n_params} parameters')
    samples = load_samples_from_dir(exp / cfg.training.sampler._dir_name, spec)       # [C, S, d]
    if args.crps and crps_refusal(cfg.data.task, samples.shape[0]):
        raise SystemExit(crps_refusal(cfg.data.task, samples.shape[0]))
    if args.stacking and stacking_refusal(samples.shape[0], samples.shape[1]):
        raise SystemExit(stacking_refusal(samples.shape[0], samples.shape[1]))
    bad_chains = ~np.isfinite(samples).all(axis=(1, 2))
    if args.drop_nonfinite and bad_chains.any() and not bad_chains.all():
        samples = samples[~bad_chains]
    x = getattr(tr.loader, f'{args.split}_x')
    y = getattr(tr.loader, f'{args.split}_y')
    x = np.ascontiguousarray(x).reshape(len(x), -1)
    eng = tr.prob_model.engine(torch.from_numpy(np.ascontiguousarray(tr.loader.train_x).reshape(len(tr.loader.train_x), -1)),
                               torch.from_numpy(np.ascontiguousarray(tr.loader.train_y)), device=args.device)
    pw = eng.pointwise_loglik(torch.from_numpy(samples), torch.from_numpy(x), torch.from_numpy(np.ascontiguousarray(y)))
    out = {'experiment': cfg.experiment_name, 'split': args.split, 'n_chains': int(samples.shape[0]),
           'n_samples': int(samples.shape[1]), 'n_points': int(x.shape[0]),
           'lppd': float(lppd(pw).item()), 'nll_mean': float(-pw.mean().item()),
           'running_lppd_last': float(running_lppd(pw)[-1].item()),
           'nonfinite_chains_total': int(bad_chains.sum()), 'nonfinite_samples': int((~torch.isfinite(torch.from_numpy(samples)).all(dim=-1)).sum().item())}
    # per chain (src/inference/evaluation.py:520-529 prints the same per-chain LPPD): the ensemble figure above is a logsumexp
    # over all chains, which a few chains thrown into a bad region (profiles/r03/01_*) barely move -- their own LPPD shows them
    kept_ids = np.arange(len(bad_chains))[~bad_chains] if (args.drop_nonfinite and bad_chains.any() and not bad_chains.all()) \
        else np.arange(len(bad_chains))
    pc = [float(lppd(pw[c:c + 1]).item()) for c in range(pw.shape[0])]
    out['chain_ids'] = [int(c) for c in kept_ids]
    out['per_chain_lppd'] = pc
    out['per_chain_lppd_median'] = float(np.nanmedian(pc))
    # RMSE of the posterior-mean prediction (src/inference/evaluation.py:509-518: mean over (chain, sample) of the predicted
    # mean, regression FCNs): a plain torch forward of the Dense stack on the device -- evaluation tooling, not the hot path
    if cfg.data.task == 'regr' and cfg.model.model == 'FCN':
        dev = torch.device(args.device)
        xt = torch.from_numpy(x).to(dev)
        flat = torch.from_numpy(samples.reshape(-1, samples.shape[-1]))
        act = {'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}[cfg.model.activation]
        leaves = {n: (o, sh) for n, o, sh in spec.leaves()}
        nl = len(spec.hidden_structure)
        mu_sum = torch.zeros(x.shape[0], dtype=torch.float64, device=dev)
        n_ok = 0
        S_ = samples.shape[1]
        mu_chain = torch.zeros((samples.shape[0], x.shape[0]), dtype=torch.float64, device=dev)     # per-chain mean prediction
        for c0 in range(0, flat.shape[0], 512):
            th = flat[c0:c0 + 512].to(dev)
            h = xt[None].expand(th.shape[0], -1, -1)
            for li in range(nl):
                ob, shb = leaves[f'fcn.layer{li}.bias']
                ok_, shk = leaves[f'fcn.layer{li}.kernel']
                h = torch.baddbmm(th[:, None, ob:ob + shb[0]], h, th[:, ok_:ok_ + shk[0] * shk[1]].reshape(-1, shk[0], shk[1]))
                if li < nl - 1:
                    h = act(h)
            mu = h[..., 0]
            fin_rows = torch.isfinite(mu).all(dim=1)
            mu_sum += mu[fin_rows].double().sum(dim=0)
            n_ok += int(fin_rows.sum())
            idx = torch.arange(c0, c0 + th.shape[0], device=dev) // S_
            mu_chain.index_add_(0, idx, torch.nan_to_num(mu.double(), nan=0.0, posinf=0.0, neginf=0.0))
        if n_ok:
            yt = torch.from_numpy(np.ascontiguousarray(y)).to(dev).double().reshape(-1)
            out['rmse'] = float(torch.sqrt(((yt - mu_sum / n_ok) ** 2).mean()).item())
            rc = torch.sqrt(((yt[None] - mu_chain / S_) ** 2).mean(dim=1))
            out['per_chain_rmse'] = [float(v) for v in rc.cpu()]
            out['per_chain_rmse_median'] = float(rc.median().item())
    out.update(predictive_metrics(eng, samples, x, np.ascontiguousarray(y), cfg.data.task, args.seed, args.coverages,
                                  with_rmse=not (cfg.data.task == 'regr' and cfg.model.model == 'FCN')))
    # dead chains: a tuned step size of 0 / NaN in warmup_params.txt (profiles/r03/01_dead_chains_mechanism.md)
    wp = exp / 'warmup_params.txt'
    if wp.exists():
        eps = np.array([float(v) for v in wp.read_text().split('\n')[0].split(',')])
        out['dead_chains_step_size_zero_or_nan'] = int((~(np.isfinite(eps) & (eps > 0))).sum())
    # ESS and ESS/s (BASELINE.json's metric; src/inference/metrics.py:386-405 on a parameter subset): per-chain ESS of
    # each selected parameter, summed over chains, min / median over the subset, per second of `time.sampling`
    from mile_amd.metrics import effective_sample_size
    fin = np.isfinite(samples).all(axis=(1, 2))             # (samples may already have been filtered by --drop-nonfinite)
    ok = samples[fin] if (fin.any() and not fin.all()) else samples
    rng = np.random.default_rng(0)
    cols = np.sort(rng.choice(samples.shape[2], size=min(args.ess_params, samples.shape[2]), replace=False))
    if ok.shape[1] >= 8:
        ess = effective_sample_size(torch.from_numpy(np.ascontiguousarray(ok[:, :, cols])).to(args.device)).sum(dim=0).cpu().numpy()
        t_sampling = None
        log = exp / 'training.log'
        if log.exists():
            import re
            m = re.findall(r'time\.sampling took ([0-9.]+) seconds', log.read_text())
            t_sampling = float(m[-1]) if m else None
        out.update({'ess_params': int(len(cols)), 'ess_min': float(np.nanmin(ess)), 'ess_median': float(np.nanmedian(ess)),
                    'time_sampling_s': t_sampling,
                    'ess_per_s_min': float(np.nanmin(ess) / t_sampling) if t_sampling else None,
                    'ess_per_s_median': float(np.nanmedian(ess) / t_sampling) if t_sampling else None})
    diag, diag_arrays = diagnostic_metrics(samples, spec, args.diagnostics, args.device)
    out.update(diag)
    if diag_arrays is not None:
        np.savez(exp / 'diagnostics.npz', **diag_arrays)
    tail_arrays = {}
    if args.tail_diagnostics is not None:
        keys, tail_arrays = tail_diagnostic_metrics(samples, args.tail_diagnostics, args.device)
        out.update(keys)
    if args.function_diagnostics is not None:
        keys, arrays, *tail = function_diagnostic_metrics(eng, samples, x, np.ascontiguousarray(y), cfg.data.task,
                                                          args.function_diagnostics, args.tail_diagnostics)
        out.update(keys)
        np.savez(exp / 'function_diagnostics.npz', **arrays)
        for tk, ta in tail:
            out.update(tk)
            tail_arrays.update(ta)
    if args.canonical_diagnostics is not None:
        keys, arrays, *tail = canonical_diagnostic_metrics(samples, spec, args.canonical_diagnostics, args.canonical_key,
                                                           args.canonical_sign, args.device, args.tail_diagnostics)
        out.update(keys)
        np.savez(exp / 'canonical_diagnostics.npz', **arrays)
        for tk, ta in tail:
            out.update(tk)
            tail_arrays.update(ta)
    if args.aligned_diagnostics is not None:
        keys, arrays, *tail = aligned_diagnostic_metrics(samples, spec, args.aligned_diagnostics, align_reference, args.align_rounds,
                                                         args.align_sign, args.device, args.tail_diagnostics)
        out.update(keys)
        np.savez(exp / 'aligned_diagnostics.npz', **arrays)
        for tk, ta in tail:
            out.update(tk)
            tail_arrays.update(ta)
    if tail_arrays:
        np.savez(exp / 'tail_diagnostics.npz', **tail_arrays)
    if args.moments:
        mom, dropped = eng.predict_moments(torch.from_numpy(samples), torch.from_numpy(x), return_dropped=True)
        keys, arrays = moment_metrics(mom, dropped, np.ascontiguousarray(y), cfg.data.task)
        out.update(keys)
        np.savez(exp / 'moments.npz', **arrays)
    if args.sensitivities:
        res = eng.predict_sensitivities(torch.from_numpy(samples), torch.from_numpy(x))
        keys, arrays = sensitivity_metrics(res, feature_labels(getattr(cfg.data, 'features', None), x.shape[1]))
        out.update(keys)
        np.savez(exp / 'sensitivities.npz', **arrays)
    if args.partial_dependence is not None:
        from mile_amd.metrics import pd_grid
        feats = list(range(x.shape[1])) if args.pd_features is None else args.pd_features
        if len(set(feats)) != len(feats) or min(feats) < 0 or max(feats) >= x.shape[1]:
            raise SystemExit(f'--pd-features: distinct indices in 0 .. {x.shape[1] - 1} are needed')
        grid = pd_grid(x, feats, args.partial_dependence)
        res = eng.predict_partial_dependence(torch.from_numpy(samples), torch.from_numpy(x), feats, grid)
        keys, arrays = partial_dependence_metrics(res, grid, feats, feature_labels(getattr(cfg.data, 'features', None), x.shape[1]))
        out.update(keys)
        np.savez(exp / 'partial_dependence.npz', **arrays)
    if args.running is not None:
        from mile_amd.metrics import curve_points, streamed_lppd
        res = streamed_lppd(eng, torch.from_numpy(samples), torch.from_numpy(x), torch.from_numpy(np.ascontiguousarray(y)),
                            curve_points=curve_points(samples.shape[1], args.running))
        keys, arrays = running_metrics(res)
        out.update(keys)
        np.savez(exp / 'running_lppd.npz', **arrays)
    if args.intervals:
        from mile_amd.metrics import interval_levels
        levels = interval_levels(args.coverages)
        quant, pit, dropped = eng.predict_quantiles(torch.from_numpy(samples), torch.from_numpy(x), levels,
                                                    y=torch.from_numpy(np.ascontiguousarray(y)), return_dropped=True)
        keys, arrays = interval_metrics(quant, pit, dropped, levels, args.coverages)
        out.update(keys)
        np.savez(exp / 'intervals.npz', **arrays)
    if args.loo:
        train_x = np.ascontiguousarray(tr.loader.train_x).reshape(len(tr.loader.train_x), -1)
        rows = eng.loo_stream(torch.from_numpy(samples), torch.from_numpy(train_x), torch.from_numpy(np.ascontiguousarray(tr.loader.train_y)),
                              r_eff=args.loo_r_eff)
        keys, arrays = loo_metrics(rows)
        out.update(keys)
        np.savez(exp / 'loo.npz', **arrays)
    if args.loo_predict:
        from mile_amd.metrics import loo_predict
        train_x = np.ascontiguousarray(tr.loader.train_x).reshape(len(tr.loader.train_x), -1)
        train_y = np.ascontiguousarray(tr.loader.train_y)
        rows = loo_predict(eng, torch.from_numpy(samples), torch.from_numpy(train_x), torch.from_numpy(train_y), r_eff=args.loo_r_eff)
        keys, arrays = loo_predict_metrics(rows, train_y, cfg.data.task, args.coverages)
        out.update(keys)
        np.savez(exp / 'loo_predict.npz', **arrays)
    if args.stacking:
        st = torch.from_numpy(samples)
        train_x = np.ascontiguousarray(tr.loader.train_x).reshape(len(tr.loader.train_x), -1)
        train_rows = eng.chain_loo_stream(st, torch.from_numpy(train_x), torch.from_numpy(np.ascontiguousarray(tr.loader.train_y)),
                                          r_eff=args.loo_r_eff, outputs=('elpd_loo', 'khat'))
        lpd_eval = eng.chain_loo_stream(st, torch.from_numpy(x), torch.from_numpy(np.ascontiguousarray(y)), outputs=('lppd',))['lppd']
        keys, arrays = stacking_metrics(train_rows, lpd_eval, eval=eng.stack_eval)
        out.update(keys)
        np.savez(exp / 'stacking.npz', **arrays)
        w_stacked = stacked_weights(arrays['weights'])
        if args.intervals:      # the stacked counterparts, next to the ensemble's keys and arrays above
            quant, pit = eng.predict_quantiles_weighted(st, torch.from_numpy(x), w_stacked, levels,
                                                        y=torch.from_numpy(np.ascontiguousarray(y)))
            keys, more = stacked_interval_metrics(quant, pit, levels, args.coverages)
            out.update(keys)
            with np.load(exp / 'intervals.npz') as z:
                np.savez(exp / 'intervals.npz', **{k: z[k] for k in z.files}, **more)
        if args.moments and cfg.data.task == 'regr':
            from mile_amd.metrics import rmse_from_moments, weighted_moments
            mom = weighted_moments(*eng.predict_moments_by_chain(st, torch.from_numpy(x)), w_stacked, cfg.data.task).cpu()
            fin = torch.isfinite(mom[:, 0])
            yt = torch.as_tensor(np.ascontiguousarray(y), dtype=torch.float64).reshape(-1)
            out['moments_stacked_rmse'] = float(rmse_from_moments(yt[fin], mom[fin])) if bool(fin.any()) else float('nan')
    if args.crps:
        from mile_amd.metrics import crps_thin_stride
        k = crps_thin_stride(samples.shape[0], samples.shape[1], args.crps_max_draws)
        thin = np.ascontiguousarray(samples[:, ::k])
        stacked = np.clip(arrays['weights'], 0.0, None) if args.stacking else None      # (stacking.npz's, just solved)
        C_ = thin.shape[0]
        W = np.stack([np.full(C_, 1.0 / C_)] + ([stacked / stacked.sum()] if stacked is not None else []))
        print(f'--crps: {C_} chains x {thin.shape[1]} draws (every {k}th of {samples.shape[1]}) on {x.shape[0]} rows')
        rows = eng.crps_stream(torch.from_numpy(thin), torch.from_numpy(x), torch.from_numpy(np.ascontiguousarray(y)), weights=W,
                               outputs=crps_outputs(x.shape[0], C_))
        keys, arrays = crps_metrics(rows, k, stacked=W[1] if stacked is not None else None)
        out.update(keys)
        np.savez(exp / 'crps.npz', **arrays)
    if args.calibration is not None:
        xt, yt = torch.from_numpy(x), torch.from_numpy(np.ascontiguousarray(y))
        if spec.hidden_structure[-1] <= 64:
            res = eng.calibration_stream(torch.from_numpy(samples), xt, yt, coverages=args.coverages, n_bins=args.calibration)
        else:                                                              # more classes than the kernels take: the torch form
            from mile_amd.metrics import classification_calibration
            res = classification_calibration(eng.predict(torch.from_numpy(samples), xt), yt.to(args.device), args.coverages, args.calibration)
        keys, arrays = calibration_metrics(res, args.calibration)
        keys['calibration_dropped'] = int(samples.shape[0] * samples.shape[1] * x.shape[0] - int(arrays['kept'][-1].sum()))
        if args.stacking:
            keys.update(stacked_calibration_metrics(res, w_stacked, yt, args.calibration))
        out.update(keys)
        np.savez(exp / 'calibration.npz', **arrays)
    (exp / 'metrics.json').write_text(json.dumps(out, indent=1) + '\n')
    print(json.dumps({k: v for k, v in out.items() if not isinstance(v, (list, dict))}))        # the per-chain arrays stay in metrics.json


if __name__ == '__main__':
    main()
