"""fp64 NumPy restatement of stacking (include/mile_hip.h, mile_stack_eval; mile_amd.metrics.stacking_weights): the definition
a row at a time, the solver, a plain multiplicative-update loop as an independent lower bound on the optimum, and the seeded
synthetic [C, N] matrices the tests share."""
from __future__ import annotations

import math

import numpy as np

FAMILIES = ('distinct', 'near_identical', 'constant', 'duplicated')
HOST_SHAPES = ((1, 5), (3, 7), (12, 1052), (64, 65), (128, 200))


def make_case(family: str, C: int, N: int, seed: int = 0) -> np.ndarray:
    """lpd [C, N] fp64: Normal log densities of N targets under C predictors.
    distinct: every chain its own bias, slope and scale; near_identical: one predictor, the chains 1e-6 apart;
    constant: as distinct, chain 0 (and every fifth) the same density on every row; duplicated: as distinct, chain 1 a copy of
    chain 0 (the Hessian is singular)."""
    rng = np.random.default_rng(1000 * seed + 31 * C + N)
    f = rng.standard_normal(N)
    y = f + 0.5 * rng.standard_normal(N)
    slope = 1.0 + 0.6 * rng.standard_normal(C)
    bias = 0.4 * rng.standard_normal(C)
    scale = np.exp(0.3 * rng.standard_normal(C)) * 0.7
    mu = slope[:, None] * f[None] + bias[:, None] + 0.3 * rng.standard_normal((C, N))
    lpd = -0.5 * ((y[None] - mu) / scale[:, None]) ** 2 - np.log(scale)[:, None] - 0.5 * math.log(2 * math.pi)
    if family == 'distinct':
        return lpd
    if family == 'near_identical':
        return lpd[:1] + 1e-6 * rng.standard_normal((C, N))
    if family == 'constant':
        lpd[::5] = -1.4 - 0.05 * np.arange(len(lpd[::5]))[:, None]
        return lpd
    if family == 'duplicated':
        if C > 1:
            lpd[1] = lpd[0]
        return lpd
    raise ValueError(family)


def stack_eval_ref(lpd, w) -> dict:
    """The definition, a row at a time: score, row_score [N], grad [C], hess [C, C], used."""
    lpd = np.asarray(lpd, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    C, N = lpd.shape
    row = np.full(N, np.nan)
    tot, g, H, used = 0.0, np.zeros(C), np.zeros((C, C)), 0
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for n in range(N):
            l = lpd[:, n]
            if np.isnan(l).any() or (l == np.inf).any():
                continue
            m = l.max()
            if not m > -np.inf:
                continue
            e = np.exp(l - m)
            mix = 0.0
            for c in range(C):
                mix += w[c] * e[c]
            row[n] = m + np.log(mix)
            R = e / mix
            used += 1
            tot += row[n]
            g += R
            H += np.outer(R, R)
        if used == 0:
            return {'score': np.nan, 'row_score': row, 'grad': np.full(C, np.nan), 'hess': np.full((C, C), np.nan), 'used': 0}
        return {'score': tot / used, 'row_score': row, 'grad': g / used, 'hess': H / used, 'used': used}


def _eval_fast(lpd, w, need_hess=True):
    """stack_eval_ref's score, grad and hess with the rows vectorised (the solver below calls it many times)."""
    ok = ~(np.isnan(lpd) | (lpd == np.inf)).any(axis=0) & (np.nan_to_num(lpd, nan=-np.inf).max(axis=0) > -np.inf)
    l = lpd[:, ok]
    m = l.max(axis=0)
    e = np.exp(l - m[None])
    mix = w @ e
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        score = float((m + np.log(mix)).sum() / l.shape[1])
        if not need_hess:
            return score, None, None
        R = e / mix[None]
        return score, R.sum(axis=1) / l.shape[1], (R @ R.T) / l.shape[1]


def qp_ref(H, g, w):
    """min 1/2 y'Hy + (1 - g - Hw)'y over y >= 0 from y = w: active set, ridge 1e-12 on the free block."""
    C = len(w)
    q = 1.0 - g - H @ w
    y = w.copy()
    free = y > 0
    for _ in range(4 * C + 16):
        F = np.flatnonzero(free)
        z = np.zeros(C)
        if F.size:
            z[F] = np.linalg.solve(H[np.ix_(F, F)] + 1e-12 * np.eye(F.size), -q[F])
        if F.size and (z[F] < 0).any():
            neg = F[z[F] < 0]
            ratio = y[neg] / np.maximum(y[neg] - z[neg], 1e-300)
            k = int(np.argmin(ratio))
            y = np.maximum(y + float(ratio[k]) * (z - y), 0.0)
            y[neg[k]] = 0.0
            free[neg[k]] = False
            y[~free] = 0.0
            continue
        y = z
        lam = H @ y + q
        lam[free] = 0.0
        k = int(np.argmin(lam))
        if lam[k] >= -1e-12:
            break
        free[k] = True
    return y


def stacking_weights_ref(lpd, tol=1e-8, max_iter=50, w0=None) -> dict:
    lpd = np.asarray(lpd, dtype=np.float64)
    C = lpd.shape[0]
    w = np.full(C, 1.0 / C) if w0 is None else np.asarray(w0, dtype=np.float64).copy()
    iters = evals = 0
    while True:
        score, g, H = _eval_fast(lpd, w)
        if not math.isfinite(score):
            return {'w': w, 'score': score, 'gap': math.inf, 'iterations': iters, 'score_evals': evals, 'converged': False}
        gap = float(g.max() - 1.0)
        if gap <= tol or iters >= max_iter:
            return {'w': w, 'score': score, 'gap': gap, 'iterations': iters, 'score_evals': evals, 'converged': gap <= tol}
        p = qp_ref(H, g, w) - w
        slope = float((1.0 - g) @ p)
        phi0 = -score + w.sum()
        t, placed = 1.0, False
        for _ in range(60):
            wt = np.maximum(w + t * p, 0.0)
            st = _eval_fast(lpd, wt, need_hess=False)[0]
            evals += 1
            if math.isfinite(st) and -st + wt.sum() <= phi0 + 1e-4 * t * slope:
                placed = True
                break
            t *= 0.5
        if not placed or not wt.sum() > 0 or np.array_equal(wt / wt.sum(), w):
            return {'w': w, 'score': score, 'gap': gap, 'iterations': iters, 'score_evals': evals, 'converged': False}
        w = wt / wt.sum()
        iters += 1


def em_lower_bound(lpd, iters=2000) -> float:
    """The score after ``iters`` multiplicative updates w <- w * grad from 1 / C: never above the optimum."""
    lpd = np.asarray(lpd, dtype=np.float64)
    w = np.full(lpd.shape[0], 1.0 / lpd.shape[0])
    for _ in range(iters):
        _, g, _ = _eval_fast(lpd, w)
        w = w * g
        w /= w.sum()
    return _eval_fast(lpd, w, need_hess=False)[0]


def support_condition(lpd, w, floor=1e-10) -> float:
    """Condition number of the Hessian restricted to the support of w (entries above ``floor``)."""
    _, _, H = _eval_fast(np.asarray(lpd, dtype=np.float64), np.asarray(w, dtype=np.float64))
    F = np.flatnonzero(np.asarray(w) > floor)
    return float(np.linalg.cond(H[np.ix_(F, F)]))
