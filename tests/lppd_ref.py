"""fp64 NumPy restatement of mile_lppd_stream: a pointwise log-likelihood tensor [C, S, N] -> the outputs of the streamed call.

NaN rule: a NaN entry is left out of its (chain, row) and counted; +inf and -inf take part as values.  A (chain, row) without
a draw makes that chain's figures NaN; the ensemble figures skip that chain on that row."""
import numpy as np


def _lse(a, axis):
    """log sum exp along ``axis``; NaN entries count as log 0.  (np.logaddexp handles equal infinities.)"""
    a = np.where(np.isnan(a), -np.inf, a)
    with np.errstate(invalid='ignore'):
        return np.logaddexp.reduce(a, axis=axis)


def _at(pw, k):
    """(chain term [C, N], ensemble term [N]) of the first k draws of every chain."""
    head = pw[:, :k]
    cnt = (~np.isnan(head)).sum(axis=1)                               # [C, N]
    A = _lse(head, axis=1)                                            # [C, N]
    with np.errstate(divide='ignore', invalid='ignore'):
        chain = np.where(cnt > 0, A - np.log(np.maximum(cnt, 1)), np.nan)
        tot = cnt.sum(axis=0)
        ens = _lse(np.where(cnt > 0, A, np.nan), axis=0) - np.log(np.maximum(tot, 1))
    return chain, np.where(tot > 0, ens, np.nan)


def ref_lppd_stream(pw, curve_points):
    """pw [C, S, N] -> dict(run_chain [K], run_ens [K], chain_lppd [C], row_lppd [N], lppd, dropped [C])."""
    pw = np.asarray(pw, dtype=np.float64)
    S = pw.shape[1]
    run_chain, run_ens = [], []
    for k in curve_points:
        chain, ens = _at(pw, int(k))
        run_chain.append(chain.mean(axis=1).mean())
        run_ens.append(ens.mean())
    chain, ens = _at(pw, S)
    return {'run_chain': np.array(run_chain, dtype=np.float64), 'run_ens': np.array(run_ens, dtype=np.float64),
            'chain_lppd': chain.mean(axis=1), 'row_lppd': ens, 'lppd': ens.mean(),
            'dropped': np.isnan(pw).sum(axis=(1, 2)).astype(np.int64)}
