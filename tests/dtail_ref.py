"""fp64 NumPy restatement of the tail diagnostics stated in include/mile_hip.h (mile_chain_diagnostics_tail): the order
statistics, the derived series, the multi-chain ESS on the split pieces (oracle.mclmc_oracle.effective_sample_size, with
the NaN rule for a weighted variance that is not a positive finite number) and the outputs, on x [C, S, d] float32.
`score_dtype` exists for the yardsticks of tests/test_gpu_dtail.py: fp64 formulas on normal scores rounded to float32."""
from __future__ import annotations

import warnings

import numpy as np

import diag_ref as R
from oracle.mclmc_oracle import effective_sample_size as _ess_mc

SERIES = ('z', 'i_lo', 'i_hi', 'x')


def quantile_indices(n):
    """Positions in the n pooled sorted draws: q_lo, q_hi, lower middle, upper middle (integers only)."""
    return (n + 19) // 20 - 1, (19 * n + 19) // 20 - 1, (n - 1) // 2, n // 2


def order_statistics(x):
    """x [C, S, d] float32 -> quantiles [3, d] float32: q_lo, q_hi, m32; NaN for a column with a NaN draw."""
    x = np.asarray(x, np.float32)
    n = x.shape[0] * x.shape[1]
    xs = np.sort(x.reshape(n, -1), axis=0)
    lo, hi, a, b = quantile_indices(n)
    with np.errstate(all='ignore'):
        m32 = ((xs[a].astype(np.float64) + xs[b].astype(np.float64)) / 2).astype(np.float32)
    q = np.stack([xs[lo], xs[hi], m32])
    q[:, np.isnan(xs[-1])] = np.nan
    return q


def series(x, score_dtype=np.float64):
    """x [C, S, d] float32 -> {'z', 'i_lo', 'i_hi', 'x', 'zf'} as float64 [C, S, d], and 'quantiles' [3, d] float32."""
    x = np.asarray(x, np.float32)
    q = order_statistics(x)
    with np.errstate(all='ignore'):
        f = np.abs(x - q[2])                                        # float32: one subtraction
        out = {'z': R._pooled_scores(x.astype(np.float64), score_dtype), 'zf': R._pooled_scores(f.astype(np.float64), score_dtype),
               'i_lo': (x <= q[0]).astype(np.float64), 'i_hi': (x <= q[1]).astype(np.float64), 'x': x.astype(np.float64)}
    out['quantiles'] = q
    return out


def _pieces(v, n_splits):
    C, S = v.shape[:2]
    return np.asarray(v, np.float64).reshape(C * n_splits, S // n_splits, -1)


def weighted_var(v, n_splits):
    p = _pieces(v, n_splits)
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        wv = p.var(axis=1).mean(axis=0)
        if p.shape[0] > 1:
            wv = wv + p.mean(axis=1).var(axis=0, ddof=1)
    return wv


def ess_mc(v, n_splits):
    """v [C, S, d] -> ESS_mc [d] on the C * n_splits pieces; NaN where weighted_var is not a positive finite number."""
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ess = _ess_mc(_pieces(v, n_splits)).reshape(-1)
        wv = weighted_var(v, n_splits)
    return np.where((wv > 0) & np.isfinite(wv), ess, np.nan)


def series_ess(x, n_splits, score_dtype=np.float64):
    """ESS_mc of the four series, [4, d] in the order of SERIES."""
    s = series(x, score_dtype)
    return np.stack([ess_mc(s[k], n_splits) for k in SERIES])


def tail_diagnostics(x, n_splits=2, score_dtype=np.float64, rhat_dtype=np.float64):
    s = series(x, score_dtype)
    e = {k: ess_mc(s[k], n_splits) for k in SERIES}
    x64 = s['x'].reshape(-1, s['x'].shape[2])
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        sd = x64.std(axis=0, ddof=1)
        tail = np.where(np.isnan(e['i_lo']) | np.isnan(e['i_hi']), np.nan, np.minimum(e['i_lo'], e['i_hi']))
        rf = R.gelman_split_r_hat(s['zf'], n_splits, rank_normalize=False, dtype=rhat_dtype)
        return {'ess_bulk': e['z'], 'ess_tail': tail, 'ess_mean': e['x'], 'mcse_mean': sd / np.sqrt(e['x']),
                'rhat_folded': np.asarray(rf, np.float64), 'quantiles': s['quantiles'], 'sd': sd}


def min_pair_mc(v, n_splits):
    """Per column: the smallest |pair sum| up to and including the truncating pair of the multi-chain estimator on the
    pieces of v [C, S, d] -- the counterpart of diag_ref.geyer_min_pair; the ESS is discontinuous where it is tiny.  inf for
    a column whose ESS is NaN by the weighted-variance rule (nothing to leave out there)."""
    p = _pieces(v, n_splits)
    M, L, d = p.shape
    xc = p - p.mean(axis=1, keepdims=True)
    m = 1 << int(np.ceil(np.log2(2 * L)))
    with np.errstate(all='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        f = np.fft.rfft(xc, n=m, axis=1)
        ac = (np.fft.irfft(f * np.conj(f), n=m, axis=1)[:, :L] / L).mean(axis=0)          # [L, d]
        wv = weighted_var(v, n_splits)
        L_even = L - L % 2
        rho = 1.0 - (ac[:1] * L / (L - 1.0) - ac[:L_even]) / wv
    rho[0] = 1.0
    pairs = rho[0::2] + rho[1::2]                                   # [T, d]
    out = np.full(d, np.inf)
    for k in range(d):
        if not (wv[k] > 0 and np.isfinite(wv[k])):
            continue
        pk = pairs[:, k]
        bad = np.nonzero(~(pk > 0))[0]
        stop = bad[0] if len(bad) else len(pk) - 1
        out[k] = np.min(np.abs(pk[:stop + 1]))
    return out


def series_min_pair(x, n_splits):
    """min_pair_mc of the four series, [4, d] in the order of SERIES."""
    s = series(x)
    return np.stack([min_pair_mc(s[k], n_splits) for k in SERIES])


def blockwise_ess(v, n_splits, block=64):
    """NumPy emulation of k_dtail_ess on v [C, S, d]: biased autocovariances of the pieces by direct summation, `block` lags at
    a time, no further block once one holds a pair sum that is not positive, then the Geyer tail on the lags computed.
    Returns (ess [d], lags computed [d])."""
    p = _pieces(v, n_splits)
    M, L, d = p.shape
    n = M * L
    xc = p - p.mean(axis=1, keepdims=True)
    L_even = L - L % 2
    T = L_even // 2
    ess, used = np.full(d, np.nan), np.zeros(d, int)
    for c in range(d):
        col = xc[:, :, c]
        between = p[:, :, c].mean(axis=1).var(ddof=1) if M > 1 else 0.0
        ac = np.zeros(L_even)
        wv = v0 = np.nan
        nlag = 0
        for k0 in range(0, L_even, block):
            for k in range(k0, min(k0 + block, L_even)):
                ac[k] = np.sum(col[:, :L - k] * col[:, k:]) / (L * M)
            if k0 == 0:
                v0, wv = ac[0] * L / (L - 1.0), ac[0] + between
            nlag = min(k0 + block, L_even)
            if not (wv > 0 and np.isfinite(wv)):
                break
            rho = 1.0 - (v0 - ac[k0:nlag]) / wv
            if k0 == 0:
                rho[0] = 1.0
            if not np.all(rho[0::2] + rho[1::2] > 0):
                break
        used[c] = nlag
        if not (wv > 0 and np.isfinite(wv)):
            continue
        rho = 1.0 - (v0 - ac[:nlag]) / wv
        rho[0] = 1.0
        t_star = T
        for t in range(nlag // 2):
            if not rho[2 * t] + rho[2 * t + 1] > 0:
                t_star = t
                break
        max_t = t_star - 1 if t_star > 0 else 0
        nxt, in_range = min(max_t + 1, T - 1), max_t + 1 <= T - 1
        total, prev, last = 0.0, 0.0, 0.0
        for t in range(nxt + 1):
            m = t < t_star
            re = rho[2 * t]
            me = (re > 0) if (t == nxt and in_range) else m
            ev, od = (re if me else 0.0), (rho[2 * t + 1] if m else 0.0)
            rs = ev + od
            if t == 0:
                prev = rs
            um = rs > prev
            cur = prev if um else rs
            ef, of = (0.5 * cur, 0.5 * cur) if um else (ev, od)
            total += ef + of
            if t == nxt:
                last = ef
            prev = cur
        tau = max(-1.0 + 2.0 * total - last, 1.0 / np.log10(n))
        ess[c] = n / tau
    return ess, used
