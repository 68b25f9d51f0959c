#!/usr/bin/env python3
"""Posterior-predictive moments of a finished experiment on NEW inputs (the consumer of mile_predict_moments):

    python predict.py -e results/mile_amd/<experiment> -i <table or .npz> [-o predictions.npz] [--draws-per-pass K] [--intervals C [C ...]] [--sets C [C ...]] [--weights PATH|stacking] [--sensitivities] [--partial-dependence G]

Reloads config.yaml and the samples the way evaluate.py does, applies the training normalisation the loader recorded
(normalization.npz, written by train.py) to the rows of the table, reduces all C x S draws on the device and writes, per row:

    regression       mean, epistemic_var, aleatoric_var     (target units, see below)
    classification   probs [N, K], entropy, mutual_information (nats)
    both             dropped: draws left out of the row because an output was not finite
    --intervals C..  regression: quantile_levels [Q] (the bounds of the central intervals of coverage C.. and the median) and
                     quantiles [N, Q] of the ensemble's predictive mixture, solved exactly on the device (target units)
    --sets C..       classification: set_levels [Q], class_order [N, K] (the classes by descending ensemble probability) and
                     set_size [N, Q]: the highest-probability set of level C is the first set_size entries of class_order
    --weights PATH   predict with the chain-weighted mixture sum_c w_c p_c instead of the equal-weight one: every output above is
                     that mixture's (the moments composed exactly from the chains' own, the quantiles by
                     mile_predict_quantiles_weighted, the sets from P = sum_c w_c P_c), ``dropped`` becomes [C, N] and
                     ``chain_weights`` [C] is added.  PATH: an .npz with ``weights``, a .npy or a text vector; ``stacking``:
                     <experiment>/stacking.npz, as evaluate.py --stacking wrote it.  One weight per chain LOADED: a vector of
                     another length is refused (evaluate and predict with the same --drop-nonfinite)
    --sensitivities  FCN experiments: sens_mean, sens_sd, sens_pos [N, P, F] and sens_dropped [N], the input sensitivities of the
                     equal-weight ensemble on every row (mile_predict_sensitivities): over the draws the mean and the sd of
                     d output_p / d x_f and the share of draws where it is positive; p = (mu, log sigma) for regression, the
                     class probabilities for classification.  In the table's units: d mu / d x_f is multiplied by y_std / x_std_f,
                     d log sigma / d x_f and d pi_k / d x_f are divided by x_std_f (--normalized keeps the network's units)
    --partial-dependence G  FCN experiments: the partial dependence and ICE curves of the equal-weight ensemble on the rows of the
                     table (mile_predict_partial_dependence), every feature over G values at the 5 % - 95 % quantiles of its own
                     column: pd_grid [F, G]; pd_ice_mean, pd_ice_sd [N, F, G, P], over the draws the mean and the sd of the
                     prediction of the row with feature f set to the grid value; pd_dropped [N, F]; pd_mean, pd_sd [F, G, P], the
                     partial dependence and its posterior band.  In the table's units: the grid in x's, mu in target units,
                     log sigma shifted by log y_std (--normalized keeps the network's units)

The table holds one row per input and the model's features as columns (no target column): .npy, .csv (comma), .data / .txt
(whitespace), or an .npz with an array ``x`` (images [N, C, H, W], token ids [N, T]).  Where the target was z-scored
(tabular regression with ``normalize``), y = y_std * y' + y_mean: the mean is mapped back the same way and BOTH variances are
multiplied by y_std^2.  ``--normalized`` takes rows that already are in the training normalisation and leaves the outputs in
it.
"""
import argparse
from pathlib import Path

import numpy as np
import torch


def read_table(path) -> np.ndarray:
    path = str(path)
    if path.endswith('.npz'):
        with np.load(path) as z:
            if 'x' not in z:
                raise SystemExit(f'{path}: an .npz input needs an array "x"')
            return np.asarray(z['x'], dtype=np.float32)
    if path.endswith('.npy'):
        return np.asarray(np.load(path), dtype=np.float32)
    if path.endswith('.csv'):
        return np.atleast_2d(np.loadtxt(path, delimiter=',', dtype=np.float32))
    if path.endswith('.data') or path.endswith('.txt'):
        return np.atleast_2d(np.loadtxt(path, dtype=np.float32))
    raise SystemExit(f'{path}: expected .npy, .csv, .data, .txt or .npz')


def read_weights(path, exp: Path, n_chains: int) -> np.ndarray:
    """--weights: the vector of ``path`` (``stacking``: <exp>/stacking.npz), one weight per loaded chain, float64 [C] >= 0
    summing to 1.  A solver's round-off is taken out first: entries in (-1e-9, 0) become 0 and a sum within 1e-6 of 1 is
    renormalised; anything further off is refused."""
    from mile_amd.metrics import chain_weights
    f = str(exp / 'stacking.npz') if path == 'stacking' else str(path)
    if not Path(f).exists():
        raise SystemExit(f'--weights: {f} does not exist' + (' (run evaluate.py --stacking first)' if path == 'stacking' else ''))
    if f.endswith('.npz'):
        with np.load(f) as z:
            if 'weights' not in z:
                raise SystemExit(f'--weights: {f} has no array "weights"')
            w = np.asarray(z['weights'], dtype=np.float64)
    elif f.endswith('.npy'):
        w = np.asarray(np.load(f), dtype=np.float64)
    else:
        w = np.atleast_1d(np.loadtxt(f, dtype=np.float64, delimiter=',' if f.endswith('.csv') else None))
    w = w.reshape(-1)
    if w.shape[0] != n_chains:
        raise SystemExit(f'--weights: {f} holds {w.shape[0]} weights, {n_chains} chains are loaded: one weight per chain, in the '
                         'order of the chains loaded (the same --drop-nonfinite as the run that solved them)')
    w = np.where((w < 0) & (w > -1e-9), 0.0, w)
    if abs(w.sum() - 1.0) <= 1e-6:
        w = w / w.sum()
    try:
        return chain_weights(w, n_chains).numpy()
    except ValueError as e:
        raise SystemExit(f'--weights: {f}: {e}')


def weighted_predictions(eng, samples, x, w, task, draws_per_pass):
    """The moment arrays of the chain-weighted mixture: per-chain moments on the device, composed on the host."""
    from evaluate import moment_metrics
    from mile_amd.metrics import weighted_moments
    mom, kept = eng.predict_moments_by_chain(samples, x, max_draws_per_pass=draws_per_pass)
    _, arrays = moment_metrics(weighted_moments(mom, kept, w, task), torch.zeros(1), np.zeros(len(x), dtype=np.float32), task)
    arrays['dropped'] = (samples.shape[1] - kept).cpu().numpy().astype(np.int32)
    arrays['chain_weights'] = np.asarray(w, dtype=np.float64)
    return arrays, mom, kept


def load_normalization(exp: Path, loader) -> dict:
    """normalization.npz of the experiment; an experiment trained before that file existed falls back to the statistics of
    the loader rebuilt from config.yaml (the same data and seed give the same numbers)."""
    from mile_amd.dataset import NORMALIZATION_FILE, normalization_stats
    f = exp / NORMALIZATION_FILE
    if f.exists():
        with np.load(f) as z:
            return {k: np.asarray(z[k], dtype=np.float32) for k in z.files}
    return normalization_stats(loader)


def denormalize(arrays: dict, norm: dict) -> dict:
    """Regression moments back in target units where the target was z-scored: mean * y_std + y_mean, variances * y_std^2."""
    if 'y_std' not in norm or 'mean' not in arrays:
        return arrays
    ys, ym = float(norm['y_std'].reshape(-1)[0]), float(norm['y_mean'].reshape(-1)[0])
    out = dict(arrays)
    out['mean'] = (arrays['mean'] * ys + ym).astype(np.float32)
    out['epistemic_var'] = (arrays['epistemic_var'] * ys * ys).astype(np.float32)
    out['aleatoric_var'] = (arrays['aleatoric_var'] * ys * ys).astype(np.float32)
    return out


def sensitivity_arrays(res: dict, norm: dict, task: str) -> dict:
    """sens_mean, sens_sd, sens_pos [N, P, F] and sens_dropped [N] of Engine.predict_sensitivities, in the units of the table where
    the loader normalised: the network sees x' = (x - x_mean) / x_std and, for a z-scored target, predicts mu' = (mu - y_mean) /
    y_std, so d mu / d x_f = (y_std / x_std_f) d mu' / d x'_f, while log sigma = log sigma' + log y_std and the class probabilities
    change with x only: both are divided by x_std_f.  The factors are positive: the sd scales with them and pos stays."""
    mean, sd = res['mean'].double().cpu().numpy(), res['sd'].double().cpu().numpy()
    if 'x_std' in norm:
        scale = np.ones(mean.shape[1:], dtype=np.float64) / np.asarray(norm['x_std'], dtype=np.float64).reshape(1, -1)
        if task == 'regr' and 'y_std' in norm:
            scale[0] *= float(norm['y_std'].reshape(-1)[0])
        mean, sd = mean * scale, sd * scale
    return {'sens_mean': mean.astype(np.float32), 'sens_sd': sd.astype(np.float32), 'sens_pos': res['pos'].cpu().numpy(),
            'sens_dropped': res['dropped'].cpu().numpy()}


def partial_dependence_arrays(res: dict, grid, norm: dict, task: str) -> dict:
    """pd_grid [F, G], pd_ice_mean, pd_ice_sd [N, F, G, P], pd_dropped [N, F] and pd_mean, pd_sd [F, G, P] of
    Engine.predict_partial_dependence, in the units of the table where the loader normalised: the grid value v' the network sees
    is (v - x_mean_f) / x_std_f; for a z-scored target mu = mu' y_std + y_mean and log sigma = log sigma' + log y_std, so the mean
    curves are scaled and shifted and the sd of mu is scaled by y_std; class probabilities stay.  Formed in fp64."""
    g = grid.double().cpu().numpy()
    a = {k: res[k].double().cpu().numpy() for k in ('ice_mean', 'ice_sd', 'pd_mean', 'pd_sd')}
    if 'x_std' in norm:
        g = g * np.asarray(norm['x_std'], dtype=np.float64).reshape(-1, 1) + np.asarray(norm['x_mean'], dtype=np.float64).reshape(-1, 1)
    if task == 'regr' and 'y_std' in norm:
        ys, ym = float(norm['y_std'].reshape(-1)[0]), float(norm['y_mean'].reshape(-1)[0])
        scale, shift = np.array([ys, 1.0]), np.array([ym, np.log(ys)])
        a = {k: v * scale + (shift if k.endswith('mean') else 0.0) for k, v in a.items()}
    return {'pd_grid': g.astype(np.float32), 'pd_ice_mean': a['ice_mean'].astype(np.float32), 'pd_ice_sd': a['ice_sd'].astype(np.float32),
            'pd_dropped': res['dropped'].cpu().numpy(), 'pd_mean': a['pd_mean'], 'pd_sd': a['pd_sd']}


def build_parser():
    ap = argparse.ArgumentParser(description='posterior-predictive moments of an experiment on a table of new inputs')
    ap.add_argument('--exp', '-e', required=True, help='experiment directory (holds config.yaml and samples/)')
    ap.add_argument('--input', '-i', required=True, help='table of inputs: .npy, .csv, .data, .txt, or .npz with an array x')
    ap.add_argument('--output', '-o', default=None, help='default: <experiment directory>/predictions.npz')
    ap.add_argument('--draws-per-pass', type=int, default=0, help='draws forwarded at a time (0: the library chooses)')
    ap.add_argument('--intervals', type=float, nargs='+', default=None, metavar='C',
                    help='regression: also the exact quantiles of the predictive mixture at the bounds of the central intervals of '
                         'these coverages and at the median (mile_predict_quantiles): quantile_levels [Q] and quantiles [N, Q], in '
                         'target units where the target was z-scored')
    ap.add_argument('--sets', type=float, nargs='+', default=None, metavar='C',
                    help='classification: also the highest-probability prediction sets of the ensemble at these coverage levels '
                         '(mile_calibration_stream): set_levels [Q], class_order [N, K] and set_size [N, Q]; the set of a level is the '
                         'first set_size entries of class_order')
    ap.add_argument('--weights', default=None, metavar='PATH',
                    help='chain weights (stacking): every output is the weighted mixture\'s.  An .npz with an array weights, a .npy '
                         'or a text vector with one weight per loaded chain; "stacking": <experiment>/stacking.npz')
    ap.add_argument('--sensitivities', action='store_true',
                    help='FCN experiments: also the input sensitivities of the ensemble on every row (mile_predict_sensitivities): '
                         'sens_mean, sens_sd, sens_pos [N, P, F] and sens_dropped [N], in the units of the table unless --normalized')
    ap.add_argument('--partial-dependence', type=int, default=None, metavar='G',
                    help='FCN experiments: also the partial dependence and ICE curves of the ensemble on the rows of the table '
                         '(mile_predict_partial_dependence), every feature over G grid values at the 5 %% - 95 %% quantiles of its own '
                         'column: pd_grid [F, G], pd_ice_mean, pd_ice_sd [N, F, G, P], pd_dropped [N, F] and pd_mean, pd_sd [F, G, P], '
                         'in the units of the table (mu in target units, log sigma shifted by log y_std) unless --normalized')
    ap.add_argument('--normalized', action='store_true',
                    help='the rows already are in the training normalisation; the outputs stay in it')
    ap.add_argument('--drop-nonfinite', action='store_true', help='leave out chains with non-finite samples, as evaluate.py does')
    ap.add_argument('--device', default='cuda:0')
    return ap


def main():
    args = build_parser().parse_args()
    exp = Path(args.exp)
    from evaluate import moment_metrics
    from mile_amd.callbacks import load_samples_from_dir
    from mile_amd.config import Config
    from mile_amd.trainer import BDETrainer
    cfg = Config.from_file(exp / 'config.yaml').replace(logging=False)
    tr = BDETrainer.__new__(BDETrainer)            # data + model spec only: no new experiment directory
    if args.intervals and cfg.data.task != 'regr':
        raise SystemExit('--intervals: predictive intervals are for regression experiments; this one is classification')
    if args.sets and cfg.data.task == 'regr':
        raise SystemExit('--sets: prediction sets are for classification experiments; this one is regression (--intervals is its counterpart)')
    tr.build_model(cfg)
    spec = tr.prob_model.spec
    if args.sensitivities:
        from mile_amd.spec import ModelSpec
        if not isinstance(spec, ModelSpec):
            raise SystemExit('--sensitivities: input sensitivities are for FCN (tabular) experiments; token ids and image pixels are out of scope')
    if args.partial_dependence is not None:
        from mile_amd.spec import ModelSpec
        if not isinstance(spec, ModelSpec):
            raise SystemExit('--partial-dependence: partial dependence is for FCN (tabular) experiments; token ids and image pixels are out of scope')
        if not 1 <= args.partial_dependence <= 256:
            raise SystemExit('--partial-dependence: G must be in 1 .. 256')
    samples = load_samples_from_dir(exp / cfg.training.sampler._dir_name, spec)       # [C, S, d]
    bad_chains = ~np.isfinite(samples).all(axis=(1, 2))
    if args.drop_nonfinite and bad_chains.any() and not bad_chains.all():
        samples = samples[~bad_chains]
    weights = read_weights(args.weights, exp, samples.shape[0]) if args.weights else None
    x = read_table(args.input)
    norm = {} if args.normalized else load_normalization(exp, tr.loader)
    if 'x_mean' in norm:
        if norm['x_mean'].ndim and x.shape[-1] != norm['x_mean'].shape[0]:
            raise SystemExit(f'{args.input}: {x.shape[-1]} columns, the model was trained on {norm["x_mean"].shape[0]} features')
        x = ((x - norm['x_mean']) / norm['x_std']).astype(np.float32)
    x = np.ascontiguousarray(x).reshape(len(x), -1)
    if x.shape[1] != spec.in_features:
        raise SystemExit(f'{args.input}: rows of {x.shape[1]} values, the model takes {spec.in_features}')
    eng = tr.prob_model.engine(torch.from_numpy(np.ascontiguousarray(tr.loader.train_x).reshape(len(tr.loader.train_x), -1)),
                               torch.from_numpy(np.ascontiguousarray(tr.loader.train_y)), device=args.device)
    if weights is None:
        mom, dropped = eng.predict_moments(torch.from_numpy(samples), torch.from_numpy(x), max_draws_per_pass=args.draws_per_pass,
                                           return_dropped=True)
        _, arrays = moment_metrics(mom, dropped, np.zeros(len(x), dtype=np.float32), cfg.data.task)
    else:
        arrays, mom_c, kept_c = weighted_predictions(eng, torch.from_numpy(samples), torch.from_numpy(x), weights, cfg.data.task,
                                                     args.draws_per_pass)
    arrays = denormalize(arrays, norm)
    if args.intervals:
        from mile_amd.metrics import interval_levels
        levels = torch.unique(torch.cat([interval_levels(args.intervals), torch.tensor([0.5], dtype=torch.float64)]), sorted=True)
        if weights is None:
            quant = eng.predict_quantiles(torch.from_numpy(samples), torch.from_numpy(x), levels, max_draws_per_pass=args.draws_per_pass)
        else:
            quant = eng.predict_quantiles_weighted(torch.from_numpy(samples), torch.from_numpy(x), weights, levels,
                                                   max_draws_per_pass=args.draws_per_pass)
        q = quant.double().cpu().numpy()
        if 'y_std' in norm:
            q = q * float(norm['y_std'].reshape(-1)[0]) + float(norm['y_mean'].reshape(-1)[0])
        arrays['quantile_levels'] = levels.numpy()
        arrays['quantiles'] = q.astype(np.float32)
    if args.sets:
        levels = sorted(float(c) for c in args.sets)
        if weights is not None:                                            # P = sum_c w_c P_c of the per-chain moments above
            from mile_amd.metrics import calibration_decide, weighted_class_probs
            P, kept = weighted_class_probs(mom_c[..., :-2].double(), kept_c, weights)
            res = calibration_decide(P[None], kept[None], None, levels)
        elif spec.hidden_structure[-1] <= 64:
            res = eng.calibration_stream(torch.from_numpy(samples), torch.from_numpy(x), coverages=levels, max_draws_per_pass=args.draws_per_pass)
        else:                                                              # more classes than the kernels take: the torch form
            from mile_amd.metrics import classification_calibration
            res = classification_calibration(eng.predict(torch.from_numpy(samples), torch.from_numpy(x)), None, levels)
        arrays['set_levels'] = np.asarray(levels, dtype=np.float64)
        arrays['class_order'] = res['order'].cpu().numpy()
        arrays['set_size'] = res['set_size'].cpu().numpy()
    if args.sensitivities:
        res = eng.predict_sensitivities(torch.from_numpy(samples), torch.from_numpy(x), max_draws_per_pass=args.draws_per_pass)
        arrays.update(sensitivity_arrays(res, norm, cfg.data.task))
    if args.partial_dependence is not None:
        from mile_amd.metrics import pd_grid
        feats = list(range(spec.in_features))
        grid = pd_grid(x, feats, args.partial_dependence)                  # of the rows as the network sees them
        res = eng.predict_partial_dependence(torch.from_numpy(samples), torch.from_numpy(x), feats, grid, max_draws_per_pass=args.draws_per_pass,
                                             want=('ice_mean', 'ice_sd', 'dropped', 'pd_mean', 'pd_sd'))
        arrays.update(partial_dependence_arrays(res, grid, norm, cfg.data.task))
    out = Path(args.output) if args.output else exp / 'predictions.npz'
    np.savez(out, **arrays)
    print(f'{out}: {len(x)} rows, {samples.shape[0] * samples.shape[1]} draws, {int(arrays["dropped"].sum())} dropped; '
          + ', '.join(f'{k} {tuple(v.shape)}' for k, v in arrays.items()))


if __name__ == '__main__':
    main()
