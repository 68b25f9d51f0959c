"""fp64 NumPy reference of the chain-weighted predictive quantiles and PIT (mile_mixture_quantiles_weighted): raw
[C, S, N, 2] (mu, log sigma), weights [C] >= 0 summing to 1.  On row n a draw with a non-finite output is left out, K_c counts
chain c's kept draws and
    F_n(t) = sum_c (w_c / K_c) sum_{i in c, kept} Phi((t - mu_i) / sigma_i),    sigma = clip(exp(log sigma), 1e-6, 1e6).
A chain with w_c = 0 enters no sum; a chain with w_c > 0 and K_c = 0 makes the row NaN.  The root of F_n(t) = p is bracketed
exactly by min and max of mu_i + Phi^-1(p) sigma_i over the components that carry weight (a convex combination of CDFs that
are all <= p, or all >= p, is so too) and found by 200 bisection steps."""
import numpy as np
from scipy.special import ndtr, ndtri


def components(raw, w):
    """raw [C, S, N, 2], w [C] -> mu, sigma, omega [C * S, N] fp64 (omega = w_c / K_c on the kept draws of the chains with
    w_c > 0, else 0), dropped [C, N] and the mask [N] of rows on which a weighted chain has nothing kept."""
    raw, w = np.asarray(raw), np.asarray(w, dtype=np.float64)
    C, S, N = raw.shape[:3]
    ok = np.isfinite(raw).all(axis=-1)                                      # [C, S, N]
    r = np.where(ok[..., None], raw, 0.0).astype(np.float64)
    K = ok.sum(axis=1)                                                      # [C, N]
    use = (w > 0)[:, None] & (K > 0)
    om = np.where(use, w[:, None] / np.maximum(K, 1), 0.0)[:, None, :] * ok
    bad = ((w > 0)[:, None] & (K == 0)).any(axis=0)
    return (r[..., 0].reshape(C * S, N), np.clip(np.exp(r[..., 1]), 1e-6, 1e6).reshape(C * S, N), om.reshape(C * S, N),
            (S - K).astype(np.int32), bad)


def cdf(raw, w, t):
    """F_n(t[n, ...]) for t [N] or [N, Q] (NaN on a row where a weighted chain has nothing kept)."""
    mu, sig, om, _, bad = components(raw, w)
    t = np.asarray(t, dtype=np.float64)
    ex = (slice(None), slice(None)) + (None,) * (t.ndim - 1)
    with np.errstate(invalid='ignore'):
        F = (ndtr((t[None] - mu[ex]) / sig[ex]) * om[ex]).sum(axis=0)
    return np.where(bad[(slice(None),) + (None,) * (t.ndim - 1)], np.nan, F)


def mixture_sd(raw, w):
    """sd_n of the weighted mixture, [N]."""
    mu, sig, om, _, bad = components(raw, w)
    m = (om * mu).sum(axis=0)
    return np.where(bad, np.nan, np.sqrt((om * ((mu - m) ** 2 + sig ** 2)).sum(axis=0)))


def quantiles(raw, w, levels, steps=200):
    """raw [C, S, N, 2], w [C], levels [Q] -> [N, Q] fp64."""
    mu, sig, om, _, bad = components(raw, w)
    p = np.asarray(levels, dtype=np.float64)
    b = mu[..., None] + ndtri(p) * sig[..., None]                           # [C * S, N, Q]
    on = (om > 0)[..., None]
    lo = np.where(on, b, np.inf).min(axis=0)
    hi = np.where(on, b, -np.inf).max(axis=0)
    with np.errstate(invalid='ignore'):                                     # (rows with nothing kept: inf - inf)
        for _ in range(steps):
            mid = lo + 0.5 * (hi - lo)
            below = (ndtr((mid[None] - mu[..., None]) / sig[..., None]) * om[..., None]).sum(axis=0) < p[None]
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        out = lo + 0.5 * (hi - lo)
    return np.where(bad[:, None], np.nan, out)


def pit(raw, w, y):
    """F_n(y_n), [N] fp64."""
    return cdf(raw, w, np.asarray(y, dtype=np.float64))


def dropped(raw, w=None):
    """S - K_c per chain and row, int32 [C, N]."""
    return components(raw, np.ones(np.asarray(raw).shape[0]) if w is None else w)[3]
