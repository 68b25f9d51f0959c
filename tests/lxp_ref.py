"""fp64 NumPy restatement of the PSIS-LOO expectations (mile_psis_expect / mile_loo_predict_stream, metrics.psis_expect_dense):
the weights of tests/loo_ref.py's psis_row kept per draw, the tie rule, the weighted and the plain sums of per-draw columns,
and the predictive columns of the streamed call.  One row at a time, plain NumPy; no device code.

For row n: the kept draws, M, the cut, the fit and the smoothed, capped, normalised log weights lw are psis_row's (stable
argsort of r).  w = exp(lw); draws whose l have equal bits (fp32 input: the bits of the float; otherwise equal values) share
the mean of their weights; a dropped draw has weight 0; fewer than two kept: every fp64 output NaN."""
import math

import numpy as np
from scipy.special import erfc, logsumexp

from tests.loo_ref import LOG_DBL_MIN, gpdfit, tail_length


def weights_row(l, r_eff=1.0):
    """One row's log-likelihoods l [S] -> (w [S] fp64 in draw order, khat, elpd_loo, dropped)."""
    l = np.asarray(l).reshape(-1)
    keys = l.view(np.uint32) if l.dtype == np.float32 else l.astype(np.float64)
    keep = np.isfinite(l)
    dropped = int((~keep).sum())
    nan = float('nan')
    w_all = np.zeros(l.shape[0], dtype=np.float64)
    lk = l[keep].astype(np.float64)
    S = len(lk)
    if S < 2:
        return np.full(l.shape[0], nan), nan, nan, dropped
    r = -lk - np.max(-lk)
    M = tail_length(S, r_eff)
    order = np.argsort(r, kind='stable')                   # ascending: the tail is the last M
    tail = order[S - M:]
    cut = max(float(r[order[S - M - 1]]), LOG_DBL_MIN)
    ec = math.exp(cut)
    khat, sigma = gpdfit(np.exp(r[tail]) - ec)
    lw = r.copy()
    if not math.isnan(khat):
        with np.errstate(all='ignore'):
            p = (np.arange(1, M + 1) - 0.5) / M
            qv = -sigma * np.log1p(-p) if khat == 0.0 else sigma * np.expm1(-khat * np.log1p(-p)) / khat
            lw[tail] = np.log(qv + ec)
    lw = np.minimum(lw, 0.0)
    lw = lw - logsumexp(lw)
    elpd = float(logsumexp(lw + lk))
    w = np.exp(lw)
    _, inv = np.unique(keys[keep], return_inverse=True)    # the tie rule: the mean over every set of equal l
    inv = inv.reshape(-1)
    w = (np.bincount(inv, weights=w) / np.bincount(inv))[inv]
    w_all[keep] = w
    return w_all, khat, elpd, dropped


def expect(loglik, values=None, r_eff=1.0):
    """loglik [S, N] (fp32: ties by bits), values [S, N, Q] or None -> dict of expect, posterior [N, Q], ess_w, khat, elpd_loo [N]
    fp64, dropped [N] int32 and weights [N, S] fp64."""
    ll = np.asarray(loglik)
    S, N = ll.shape
    out = {k: np.empty(N) for k in ('ess_w', 'khat', 'elpd_loo')}
    out['dropped'] = np.zeros(N, dtype=np.int32)
    out['weights'] = np.empty((N, S))
    if values is not None:
        v = np.asarray(values, dtype=np.float64).reshape(S, N, -1)
        out['expect'] = np.empty((N, v.shape[2]))
        out['posterior'] = np.empty((N, v.shape[2]))
    for n in range(N):
        w, out['khat'][n], out['elpd_loo'][n], out['dropped'][n] = weights_row(ll[:, n], r_eff)
        out['weights'][n] = w
        keep = np.isfinite(ll[:, n])
        few = keep.sum() < 2
        with np.errstate(all='ignore'):
            out['ess_w'][n] = float('nan') if few else 1.0 / np.sum(w[keep] ** 2)
            if values is not None:
                h = v[keep, n, :]
                out['expect'][n] = float('nan') if few else (w[keep][:, None] * h).sum(axis=0)
                out['posterior'][n] = float('nan') if few else h.sum(axis=0) / keep.sum()
    return out


def columns(raw, y, task):
    """The predictive columns from raw outputs raw [S, N, O] (any float dtype; read as fp64): regression (mu, mu^2, sigma^2,
    Phi((y - mu) / sigma)) with sigma = exp(log sigma) clipped to [1e-6, 1e6]; classification softmax(raw)."""
    z = np.asarray(raw, dtype=np.float64)
    with np.errstate(all='ignore'):
        if task == 'regr':
            mu = z[..., 0]
            es = np.exp(z[..., 1])
            sig = np.where(np.isnan(es), es, np.clip(es, 1e-6, 1e6))
            yv = np.asarray(y, dtype=np.float64)
            return np.stack([mu, mu * mu, sig * sig, 0.5 * erfc(-((yv - mu) / sig) / math.sqrt(2.0))], axis=-1)
        m = z.max(axis=-1, keepdims=True)
        return np.exp(z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True))))
