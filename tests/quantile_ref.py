"""fp64 NumPy reference of the ensemble's predictive quantiles and PIT (mile_mixture_quantiles): on row n the predictive
is the equal-weight mixture of the kept draws' Normals, F_n(t) = mean_s Phi((t - mu_sn) / sigma_sn) with
sigma = clip(exp(log sigma), 1e-6, 1e6).  The root of F_n(t) = p is bracketed exactly by min_s and max_s of
mu_s + Phi^-1(p) sigma_s (a component's CDF at t is <= p exactly when t <= mu_s + z_p sigma_s) and found by 200 bisection
steps.  A draw with a non-finite output on a row is left out of that row; a row with nothing kept is NaN."""
import numpy as np
from scipy.special import ndtr, ndtri


def components(raw):
    """raw [S, N, 2] -> mu, sigma [S, N] in fp64 and the mask of kept draws [S, N]."""
    raw = np.asarray(raw)
    ok = np.isfinite(raw).all(axis=-1)
    r = np.where(ok[..., None], raw, 0.0).astype(np.float64)
    return r[..., 0], np.clip(np.exp(r[..., 1]), 1e-6, 1e6), ok


def cdf(raw, t):
    """F_n(t[n, ...]) for t [N] or [N, Q]: the mean of the kept components' CDFs (NaN where nothing is kept)."""
    mu, sig, ok = components(raw)
    t = np.asarray(t, dtype=np.float64)
    ex = (slice(None), slice(None)) + (None,) * (t.ndim - 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        c = ndtr((t[None] - mu[ex]) / sig[ex]) * ok[ex]
        return c.sum(axis=0) / ok.sum(axis=0)[(slice(None),) + (None,) * (t.ndim - 1)]


def mixture_sd(raw):
    """sd_n of the mixture: sqrt(Var_s mu + mean_s sigma^2) over the kept draws, [N]."""
    mu, sig, ok = components(raw)
    with np.errstate(invalid='ignore', divide='ignore'):
        k = ok.sum(axis=0)
        m = (mu * ok).sum(axis=0) / k
        return np.sqrt((((mu - m) ** 2 + sig ** 2) * ok).sum(axis=0) / k)


def quantiles(raw, levels, steps=200):
    """raw [S, N, 2], levels [Q] -> [N, Q] fp64."""
    mu, sig, ok = components(raw)
    z = ndtri(np.asarray(levels, dtype=np.float64))
    b = mu[..., None] + z * sig[..., None]                                  # [S, N, Q]
    lo = np.where(ok[..., None], b, np.inf).min(axis=0)
    hi = np.where(ok[..., None], b, -np.inf).max(axis=0)
    p = np.asarray(levels, dtype=np.float64)[None]
    with np.errstate(invalid='ignore'):                                     # (rows with nothing kept: inf - inf)
        for _ in range(steps):
            mid = lo + 0.5 * (hi - lo)
            below = cdf(raw, mid) < p
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        out = lo + 0.5 * (hi - lo)
    return np.where(ok.any(axis=0)[:, None], out, np.nan)


def pit(raw, y):
    """F_n(y_n), [N] fp64."""
    return cdf(raw, np.asarray(y, dtype=np.float64))
