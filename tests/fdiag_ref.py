"""fp64 NumPy restatement of the columns and summaries of mile_function_diagnostics (include/mile_hip.h), straight from the
definitions.  The forwards are the project's fp64 ones (oracle.mclmc_oracle.mlp_forward, tests/lenetti_ref.forward); the
statistics of the columns are tests/diag_ref.chain_diagnostics.

Columns: outputs [C, S, N, O] -> [C, S, M].  Q = O + 1 (Q = O without y); column n * Q + q is quantity q of row n --
regression (mu, log sigma, l), classification (the O softmax probabilities, l), l = log p(y_n | x_n, theta) with sigma
clipped to [1e-6, 1e6] -- and with y the last column is L = sum_n l_n, added one row after another in row order."""
from __future__ import annotations

import functools
import warnings

import numpy as np

from oracle import mclmc_oracle as O
from tests import diag_ref as R

_LOG_SQRT_2PI = 0.91893853320467274

SUMMARY = ('rhat_max', 'rhat_mean', 'rhat_column', 'rhat_gt_1_01', 'rhat_gt_1_05', 'rhat_gt_1_1', 'rhat_skipped',
           'crhat_max', 'crhat_chain', 'crhat_column', 'crhat_skipped',
           'ess_min', 'ess_mean', 'ess_chain', 'ess_column', 'ess_skipped')


def row_loglik(out, y, task):
    """out [..., N, O] fp64, y [N] -> l [..., N]."""
    out = np.asarray(out, np.float64)
    with np.errstate(all='ignore'):
        if task == 'regr':
            es = np.exp(out[..., 1])
            sig = np.where(np.isnan(es), es, np.clip(es, 1e-6, 1e6))
            r = (np.asarray(y, np.float64) - out[..., 0]) / sig
            return -0.5 * r * r - np.log(sig) - _LOG_SQRT_2PI
        m = out.max(axis=-1, keepdims=True)
        lse = m + np.log(np.exp(out - m).sum(axis=-1, keepdims=True))
        yi = np.broadcast_to(np.asarray(y, np.int64).reshape((1,) * (out.ndim - 2) + (-1, 1)), out.shape[:-1] + (1,))
        return (np.take_along_axis(out, yi, axis=-1) - lse)[..., 0]


def columns(out, y, task):
    """out [C, S, N, O] fp64 -> ([C, S, M] fp64, L [C, S] fp64 or None)."""
    out = np.asarray(out, np.float64)
    C, S, N, O = out.shape
    with np.errstate(all='ignore'):
        if task == 'regr':
            head = out
        else:
            m = out.max(axis=-1, keepdims=True)
            head = np.exp(out - (m + np.log(np.exp(out - m).sum(axis=-1, keepdims=True))))
    if y is None:
        return head.reshape(C, S, N * O), None
    ll = row_loglik(out, y, task)
    L = np.zeros((C, S))
    for n in range(N):                                    # row order; a NaN l makes L NaN
        L = L + ll[:, :, n]
    cols = np.concatenate([head, ll[..., None]], axis=-1).reshape(C, S, N * (O + 1))
    return np.concatenate([cols, L[:, :, None]], axis=-1), L


def summaries(rhat, crhat, ess, NQ):
    """The summary (dict keyed by SUMMARY) and chain_summary [C, 2] of given statistic arrays over their first NQ columns.
    Non-finite cells are skipped and counted; of equal extremes the lower chain, then the lower column wins; means are
    float64 sums over the finite cells; NaN and -1 where no cell is finite."""
    r = np.asarray(rhat, np.float64)[:NQ]
    c = np.asarray(crhat, np.float64)[:, :NQ]
    e = np.asarray(ess, np.float64)[:, :NQ]
    s = {}
    fr = np.isfinite(r)
    best, col = np.nan, -1
    for i in range(NQ):
        if fr[i] and (col < 0 or r[i] > best):
            best, col = r[i], i
    s['rhat_max'], s['rhat_column'] = best, col
    s['rhat_mean'] = r[fr].sum() / fr.sum() if fr.any() else np.nan
    for name, thr in (('rhat_gt_1_01', 1.01), ('rhat_gt_1_05', 1.05), ('rhat_gt_1_1', 1.1)):
        s[name] = int((r[fr] > thr).sum())
    s['rhat_skipped'] = int((~fr).sum())
    chain = np.full((c.shape[0], 2), np.nan)
    for key, a, larger, k in (('crhat_max', c, True, 1), ('ess_min', e, False, 0)):
        best, at = np.nan, (-1, -1)
        for ch in range(a.shape[0]):
            for i in range(NQ):
                v = a[ch, i]
                if not np.isfinite(v):
                    continue
                if np.isnan(chain[ch, k]) or (v > chain[ch, k] if larger else v < chain[ch, k]):
                    chain[ch, k] = v
                if at[0] < 0 or (v > best if larger else v < best):
                    best, at = v, (ch, i)
        stem = key.split('_')[0]
        s[key], s[f'{stem}_chain'], s[f'{stem}_column'] = best, at[0], at[1]
        s[f'{stem}_skipped'] = int((~np.isfinite(a)).sum())
    fe = np.isfinite(e)
    s['ess_mean'] = e[fe].sum() / fe.sum() if fe.any() else np.nan
    return s, chain


def permuted_mode_draws(leaves, d, widths, C, S, seed, scale=0.05, centre_scale=0.7):
    """The permutation case: C chains of S i.i.d. draws N(centre, scale^2) around ONE centre of a [F -> H -> H -> O] net, chain
    c > 0 with the units of the first hidden layer permuted (layer0's bias and kernel columns, layer1's kernel rows): the same
    functions, other parameters.  `leaves`: [(name, offset, shape)] of the project's layout with names ending in
    layer<i>.bias / layer<i>.kernel.  Returns theta [C, S, d] fp64."""
    rng = np.random.default_rng(seed)
    off = {n.split('.', 1)[1]: (o, sh) for n, o, sh in leaves}
    centre = centre_scale * rng.standard_normal(d)
    theta = centre + scale * rng.standard_normal((C, S, d))
    H = widths[0]
    for c in range(1, C):
        perm = rng.permutation(H)
        while (perm == np.arange(H)).any():               # a derangement: every unit moves
            perm = rng.permutation(H)
        t = theta[c].copy()
        ob, _ = off['layer0.bias']
        theta[c][:, ob:ob + H] = t[:, ob:ob + H][:, perm]
        ok, sh = off['layer0.kernel']
        theta[c][:, ok:ok + sh[0] * sh[1]] = t[:, ok:ok + sh[0] * sh[1]].reshape(S, sh[0], sh[1])[:, :, perm].reshape(S, -1)
        ok, sh = off['layer1.kernel']
        theta[c][:, ok:ok + sh[0] * sh[1]] = t[:, ok:ok + sh[0] * sh[1]].reshape(S, sh[0], sh[1])[:, perm, :].reshape(S, -1)
    return theta


# the permutation case of the tests: [3 -> 8 -> 8 -> 2] tanh regression, 3 chains of 64 draws, 5 rows
PERM_WIDTHS, PERM_C, PERM_S, PERM_N, PERM_SEED = (8, 8, 2), 3, 64, 5, 0


@functools.lru_cache(maxsize=None)
def permutation_case(leaves):
    """leaves: the project's leaf layout of the net as a tuple.  Returns theta [C, S, d] fp64, X, y (fp32), the oracle's spec,
    the fp64 columns and the fp64 function-space and parameter-space diagnostics (computed once, shared, never changed)."""
    ospec = O.ModelSpec(3, PERM_WIDTHS, activation='tanh', task='regr')
    d = ospec.n_params
    theta = permuted_mode_draws(leaves, d, PERM_WIDTHS, PERM_C, PERM_S, PERM_SEED)
    rng = np.random.default_rng(PERM_SEED + 1)
    X = rng.standard_normal((PERM_N, 3)).astype(np.float32)
    y = rng.standard_normal(PERM_N).astype(np.float32)
    out = O.mlp_forward(ospec, theta.reshape(-1, d), X.astype(np.float64)).reshape(PERM_C, PERM_S, PERM_N, 2)
    cols, _ = columns(out, y, 'regr')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fn, par = R.chain_diagnostics(cols, 2), R.chain_diagnostics(theta, 2)
    for v in (theta, X, y, cols):
        v.setflags(write=False)
    return theta, X, y, ospec, cols, fn, par
