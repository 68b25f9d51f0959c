"""fp64 NumPy restatement of the reference's chain diagnostics (src/inference/metrics.py:226-244, 354-405, 449-523):
between_chain_var, within_chain_var, effective_sample_size, gelman_split_r_hat, split_chain_r_hat, all on x [C, S, ...].
The single-chain ESS is oracle.mclmc_oracle.effective_sample_size (the estimator mile_amd.diagnostics restates).
`dtype` / `score_dtype` exist for the yardsticks of tests/test_gpu_diag.py: the same formulas evaluated in float32, and
fp64 formulas on normal scores rounded to float32."""
from __future__ import annotations

import warnings

import numpy as np
from scipy.stats import norm, rankdata

from oracle.mclmc_oracle import effective_sample_size as _ess1


def ar1_draws(C, S, d, seed, ties):
    """Stationary AR(1) columns, phi ~ U(-0.5, 0.98), plus a chain offset 0.3 N(0,1) per (chain, column), as float32; with
    `ties` every fourth column is rounded to multiples of 0.25."""
    rng = np.random.default_rng(seed)
    phi = rng.uniform(-0.5, 0.98, d)
    eps = rng.standard_normal((C, S, d))
    x = np.empty((C, S, d))
    x[:, 0] = eps[:, 0] / np.sqrt(1.0 - phi ** 2)
    for t in range(1, S):
        x[:, t] = phi * x[:, t - 1] + eps[:, t]
    x += 0.3 * rng.standard_normal((C, 1, d))
    x = x.astype(np.float32)
    if ties:
        x[:, :, ::4] = np.round(x[:, :, ::4] * 4) / 4
    return x


def rank_normalize_columns(x2, score_dtype=np.float64):
    """x2 [n, ...]: each column ranked over its n entries (average rank for ties; a NaN makes the column NaN)."""
    n = x2.shape[0]
    ranks = rankdata(np.asarray(x2, np.float64), axis=0)
    return norm.ppf((ranks - 0.375) / (n + 0.25)).astype(score_dtype).astype(np.float64)


def _pooled_scores(x, score_dtype=np.float64):
    return rank_normalize_columns(x.reshape(-1, *x.shape[2:]), score_dtype).reshape(x.shape)


def between_chain_var(x):
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return x.mean(axis=1).var(axis=0, ddof=1)


def within_chain_var(x):
    with np.errstate(all='ignore'):
        return x.var(axis=1, ddof=1).mean(axis=0)


def effective_sample_size(x, rank_normalize=True, score_dtype=np.float64):
    x = np.asarray(x, np.float64)
    z = _pooled_scores(x, score_dtype) if rank_normalize else x
    with np.errstate(all='ignore'):
        return np.stack([_ess1(z[c][None]).reshape(x.shape[2:]) for c in range(x.shape[0])])


def gelman_split_r_hat(x, n_splits, rank_normalize=True, dtype=np.float64):
    C, S = x.shape[:2]
    if S % n_splits:
        raise ValueError('Number of samples must be divisible by n_splits')
    n = S // n_splits
    z = _pooled_scores(np.asarray(x, np.float64)) if rank_normalize else np.asarray(x)
    sp = z.astype(dtype).reshape(C * n_splits, n, *x.shape[2:])
    wcv, bcv = within_chain_var(sp), between_chain_var(sp)
    with np.errstate(all='ignore'):
        return np.sqrt((dtype(n - 1) / dtype(n) * wcv + bcv) / wcv)


def split_chain_r_hat(x, n_splits, rank_normalize=True, dtype=np.float64):
    return np.stack([gelman_split_r_hat(ch[None], n_splits, rank_normalize, dtype) for ch in x])


def chain_diagnostics(x, n_splits=2):
    x64 = np.asarray(x, np.float64)
    return {'wcv': within_chain_var(x64), 'bcv': between_chain_var(x64), 'ess': effective_sample_size(x64),
            'crhat': split_chain_r_hat(x64, n_splits), 'rhat': gelman_split_r_hat(x64, n_splits)}


def geyer_min_pair(x):
    """Per (chain, column): the smallest |pair sum| up to and including the truncating pair of the single-chain estimator
    on the pooled scores -- the cells where the ESS is discontinuous are those where it is tiny."""
    x = np.asarray(x, np.float64)
    C, S = x.shape[:2]
    z = _pooled_scores(x).reshape(C, S, -1)
    xc = z - z.mean(axis=1, keepdims=True)
    m = 1 << int(np.ceil(np.log2(2 * S)))
    f = np.fft.rfft(xc, n=m, axis=1)
    ac = np.fft.irfft(f * np.conj(f), n=m, axis=1)[:, :S] / S
    S_even = S - S % 2
    with np.errstate(all='ignore'):
        rho = 1.0 - (ac[:, :1] * S / (S - 1.0) - ac[:, :S_even]) / ac[:, :1]
    rho[:, 0] = 1.0
    pairs = rho[:, 0::2] + rho[:, 1::2]                       # [C, T, d]
    out = np.empty((C, pairs.shape[2]))
    for c in range(C):
        for k in range(pairs.shape[2]):
            p = pairs[c, :, k]
            bad = np.nonzero(~(p > 0))[0]
            stop = bad[0] if len(bad) else len(p) - 1
            out[c, k] = np.min(np.abs(p[:stop + 1]))
    return out.reshape(C, *x.shape[2:])
