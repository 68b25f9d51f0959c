"""fp64 NumPy restatement of PSIS-LOO and WAIC of an ensemble, one row at a time (Vehtari, Gelman & Gabry 2017; Vehtari et al.
2024; the generalised-Pareto fit of Zhang & Stephens 2009): plain loops, np.sort, scipy's logsumexp.  The checker of
mile_psis_loo / mile_loo_stream and of mile_amd.metrics.psis_loo; no device code.

For row n with l_s = log p(y_n | x_n, theta_s): a draw with a NaN or +-inf l_s is left out of the row (``dropped`` counts
them, S_n are kept; fewer than two kept: every output NaN).  lppd = logsumexp l - log S_n; p_waic = the ddof-1 variance of
l; the log ratios r = -l - max(-l); the tail the M = ceil(min(S_n / 5, 3 sqrt(S_n / r_eff))) largest r above
cut = max((M+1)-th largest r, log DBL_MIN); the fit on x = exp(r) - exp(cut); the smoothed tail, min(., 0), normalised;
elpd_loo = logsumexp(lw + l)."""
import math

import numpy as np
from scipy.special import logsumexp

LOG_DBL_MIN = math.log(np.finfo(np.float64).tiny)


def tail_length(S_n, r_eff=1.0):
    return int(math.ceil(min(S_n / 5.0, 3.0 * math.sqrt(S_n / r_eff))))


def gpdfit(x):
    """(khat, sigma) of the generalised-Pareto fit to the ascending exceedances x [M]; (nan, nan) when the fit does not run
    (M < 5, x_q <= 0) or gives a non-finite khat or sigma."""
    x = np.asarray(x, dtype=np.float64)
    M = len(x)
    nofit = (float('nan'), float('nan'))
    if M < 5:
        return nofit
    q = int(math.floor(M / 4 + 0.5))
    xq, xM = x[q - 1], x[M - 1]
    if not xq > 0.0:
        return nofit
    m = 30 + int(math.floor(math.sqrt(M)))
    with np.errstate(all='ignore'):
        b = np.empty(m)
        k = np.empty(m)
        for j in range(1, m + 1):
            b[j - 1] = (1.0 - math.sqrt(m / (j - 0.5))) / (3.0 * xq) + 1.0 / xM
            k[j - 1] = np.mean(np.log1p(-b[j - 1] * x))
        L = M * (np.log(-b / k) - k - 1.0)
        w = np.empty(m)
        for j in range(m):
            w[j] = 1.0 / np.sum(np.exp(L - L[j]))          # an overflowing term: the sum is inf and the weight 0
        bb = float(np.sum(b * w))
        kk = float(np.mean(np.log1p(-bb * x)))
        sigma = -kk / bb
        khat = (M * kk + 5.0) / (M + 10.0)
    if not (math.isfinite(khat) and math.isfinite(sigma)):
        return nofit
    return khat, sigma


def psis_row(l, r_eff=1.0):
    """(lppd, p_waic, elpd_loo, khat, dropped) of one row's log-likelihoods l [S]."""
    l = np.asarray(l, dtype=np.float64).reshape(-1)
    keep = np.isfinite(l)
    dropped = int((~keep).sum())
    l = l[keep]
    S = len(l)
    nan = float('nan')
    if S < 2:
        return nan, nan, nan, nan, dropped
    lppd = float(logsumexp(l)) - math.log(S)
    p_waic = float(np.sum((l - np.mean(l)) ** 2) / (S - 1))
    r = -l - np.max(-l)
    M = tail_length(S, r_eff)
    order = np.argsort(r, kind='stable')                   # ascending: the tail is the last M
    tail = order[S - M:]
    cut = max(float(r[order[S - M - 1]]), LOG_DBL_MIN)
    ec = math.exp(cut)
    x = np.exp(r[tail]) - ec
    khat, sigma = gpdfit(x)
    lw = r.copy()
    if not math.isnan(khat):
        with np.errstate(all='ignore'):
            p = (np.arange(1, M + 1) - 0.5) / M
            if khat == 0.0:
                qv = -sigma * np.log1p(-p)
            else:
                qv = sigma * np.expm1(-khat * np.log1p(-p)) / khat
            lw[tail] = np.log(qv + ec)
    lw = np.minimum(lw, 0.0)
    lw = lw - logsumexp(lw)
    return lppd, p_waic, float(logsumexp(lw + l)), khat, dropped


def psis_loo(loglik, r_eff=1.0):
    """loglik [S, N] (any float dtype; read as fp64) -> dict of lppd, p_waic, elpd_loo, khat [N] fp64 and dropped [N] int32."""
    ll = np.asarray(loglik)
    ll = ll.reshape(-1, ll.shape[-1]).astype(np.float64)
    N = ll.shape[1]
    out = {k: np.empty(N) for k in ('lppd', 'p_waic', 'elpd_loo', 'khat')}
    out['dropped'] = np.zeros(N, dtype=np.int32)
    for n in range(N):
        out['lppd'][n], out['p_waic'][n], out['elpd_loo'][n], out['khat'][n], out['dropped'][n] = psis_row(ll[:, n], r_eff)
    return out
