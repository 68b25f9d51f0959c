"""The exact CRPS of the predictive mixture in NumPy fp64, straight from the definitions (include/mile_hip.h,
mile_mixture_crps): the reference of the CRPS tests, from the same fp32 raw values the device reads.

raw [C, S, N, 2] (mu, log sigma), y [N], weights [n_w, C] or None.  Row 0 of the mix outputs is the pooled ensemble,
w_c = K_c / sum K.  Besides the outputs, ``t1`` = sum_c w_c a_c and ``t2`` = w'Gw per (mix row, data row) and ``t1_chain`` =
a_c, ``t2_chain`` = G_cc per (chain, row): the positive sums the error bounds are stated in.
"""
from __future__ import annotations

import numpy as np
from scipy.special import erf


def abs_normal_mean(d, v):
    """A(d, v) = E|N(d, v)| = d erf(d / sqrt(2 v)) + sqrt(2 v / pi) exp(-d^2 / (2 v))."""
    d, v = np.asarray(d, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return d * erf(d / np.sqrt(2.0 * v)) + np.sqrt(2.0 * v / np.pi) * np.exp(-d * d / (2.0 * v))


def single_normal_crps(mu, sigma, y):
    """sigma [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)], z = (y - mu) / sigma: the CRPS of one Normal (Gneiting & Raftery 2007)."""
    z = (np.asarray(y, dtype=np.float64) - mu) / sigma
    return sigma * (z * erf(z / np.sqrt(2.0)) + 2.0 * np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi) - 1.0 / np.sqrt(np.pi))


def crps(raw, y, weights=None, chunk: int = 1 << 22):
    raw = np.asarray(raw)
    C, S, N = raw.shape[:3]
    W = np.zeros((0, C)) if weights is None else np.atleast_2d(np.asarray(weights, dtype=np.float64))
    ok = np.isfinite(raw).all(axis=-1)                                      # [C, S, N]
    r = np.where(ok[..., None], raw, 0.0).astype(np.float64)
    mu = r[..., 0]
    with np.errstate(over='ignore'):
        var = np.clip(np.exp(r[..., 1]), 1e-6, 1e6) ** 2
    y = np.asarray(y, dtype=np.float64)
    K = ok.sum(axis=1).astype(np.float64)                                   # [C, N]
    with np.errstate(invalid='ignore', divide='ignore'):
        a = (abs_normal_mean(y[None, None] - mu, var) * ok).sum(axis=1) / K
        G = np.empty((N, C, C))
        step = max(1, chunk // max(1, S))
        for n in range(N):
            for c in range(C):
                mi, vi = mu[c, ok[c, :, n], n], var[c, ok[c, :, n], n]
                for c2 in range(c, C):
                    mj, vj = mu[c2, ok[c2, :, n], n], var[c2, ok[c2, :, n], n]
                    tot = 0.0
                    for i0 in range(0, len(mi), step):
                        tot += abs_normal_mean(mi[i0:i0 + step, None] - mj[None], vi[i0:i0 + step, None] + vj[None]).sum()
                    G[n, c, c2] = G[n, c2, c] = tot / (K[c, n] * K[c2, n])
        Kt = K.sum(axis=0)
        pooled = np.where(Kt > 0, K / Kt, np.nan).T                         # [N, C]
        t1 = np.empty((1 + len(W), N))
        t2 = np.empty((1 + len(W), N))
        for m in range(1 + len(W)):
            w = pooled if m == 0 else np.broadcast_to(W[m - 1], (N, C))
            ww = w[:, :, None] * w[:, None, :]
            t1[m] = np.where(w == 0, 0.0, w * a.T).sum(axis=1)
            t2[m] = np.where(ww == 0, 0.0, ww * G).sum(axis=(1, 2))
    diag = np.diagonal(G, axis1=1, axis2=2).T
    return {'crps_chain': a - 0.5 * diag, 'spread_chain': 0.5 * diag, 'crps_mix': t1 - 0.5 * t2, 'spread_mix': 0.5 * t2, 'gram': G,
            'dropped': (S - ok.sum(axis=1)).astype(np.int32), 't1': t1, 't2': t2, 't1_chain': a, 't2_chain': diag, 'pooled': pooled}
