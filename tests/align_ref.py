"""NumPy restatement of the alignment of FCN draws to a reference draw by hidden-unit assignment (mile_align_fcn,
include/mile_hip.h), straight from the rule and from ModelSpec.leaves() offsets.  No torch, no scipy.

Hidden layers l = 0 .. n_hidden - 1 are solved in ascending order.  S[i][j] (fp64) is the dot product of reference unit i's
(bias, incoming column) with draw unit j's, the draw's rows already in the previous layer's aligned order and sign, the terms
added one after another from the bias product on; the last hidden layer adds the outgoing rows.  G = S, or |S| with the sign fix
(tanh).  p_l maximises sum_i G[i][p_l[i]]: the shortest-augmenting-path Hungarian method on c = -G in a fixed operation order
(``hungarian``), additions, subtractions and comparisons only, so the device's permutation equals this one bit for bit."""
from __future__ import annotations

import functools

import numpy as np

from tests.canon_ref import _layers, orbit_member, permutation_draws, permutation_spec, random_draws

# The shapes of the tests: the smallest at which each part can go wrong.
# name: (in_features, hidden_structure, activation, task, M, noise)
CASES = {
    'sep': (3, (8, 8, 2), 'tanh', 'regr', 24, 0.05),                   # small net, sign fix
    'w64x3': (5, (64, 64, 64, 2), 'relu', 'regr', 6, 0.05),            # a full wave per layer, three chained layers
    'w128': (4, (128, 2), 'tanh', 'regr', 3, 0.05),                    # two columns per lane, one hidden layer, outgoing features
    'odd': (7, (33, 17, 5, 2), 'tanh', 'regr', 8, 0.05),               # widths below and across a wave, not powers of two
    'w16': (5, (16, 16, 2), 'relu', 'regr', 40, 0.3),                  # noise 0.3: assignments that do not recover the original
    'deep12': (4, (3,) * 11 + (2,), 'tanh', 'regr', 5, 0.05),          # twelve layers: layer10 lies before layer2
    'width1': (2, (1, 2), 'tanh', 'regr', 4, 0.05),                    # nothing to order
    'nohidden': (6, (3,), 'relu', 'classification', 4, 0.05),          # H = 0: a copy
}
RECOVERED = ('sep', 'w64x3', 'w128', 'odd')                            # alignment to the centre returns the unpermuted draws


def case_spec(name):
    from mile_amd import ModelSpec
    fin, hs, act, task, _, _ = CASES[name]
    return ModelSpec(fin, hs, activation=act, task=task)


def case_signs(name):
    """The values of ``sign`` the case runs with: the sign fix where tanh allows it."""
    return (False, True) if CASES[name][2] == 'tanh' else (False,)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(centre [d], original [M, d], moved [M, d]) fp32, computed once, never changed: noisy copies of a centre drawn at scale
    0.7, and another member of each copy's orbit (hidden units permuted, for tanh sign-flipped)."""
    spec = case_spec(name)
    M, noise = CASES[name][4], CASES[name][5]
    centre = random_draws(spec, 1, seed=5, scale=0.7)[0]
    rng = np.random.default_rng(9)
    orig = (centre[None] + noise * rng.standard_normal((M, spec.n_params))).astype(np.float32)
    moved = orbit_member(spec, orig, seed=3, flips=CASES[name][2] == 'tanh')
    for v in (centre, orig, moved):
        v.setflags(write=False)
    return centre, orig, moved


@functools.lru_cache(maxsize=None)
def case_aligned(name, sign):
    """(out, perm, sign, score, dropped) of the case's moved draws aligned to its centre."""
    centre, _, moved = case_data(name)
    res = align(case_spec(name), moved, centre, sign)
    for v in res:
        v.setflags(write=False)
    return res


def hungarian(c):
    """c [n, n] fp64 finite -> p [n]: row i takes column p[i], minimising sum_i c[i][p[i]].  Shortest augmenting paths with
    potentials, 1-based with the virtual column 0 as in the classical statement: rows inserted in ascending i; cur =
    (c[i0][j] - u[i0]) - v[j]; minv and way updated on cur < minv; the next column is the unused one with the smallest minv, the
    lowest index among equals; then u[p[j]] += delta, v[j] -= delta on used columns, minv[j] -= delta on the others."""
    n = c.shape[0]
    u, v = np.zeros(n + 1), np.zeros(n + 1)
    p, way = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    cc = np.zeros((n + 1, n + 1))
    cc[1:, 1:] = c
    for i in range(1, n + 1):
        p[0], j0 = i, 0
        minv, used = np.full(n + 1, np.inf), np.zeros(n + 1, bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            free = ~used
            cur = (cc[i0] - u[i0]) - v
            upd = free & (cur < minv)
            minv[upd], way[upd] = cur[upd], j0
            cand = np.where(free, minv, np.inf)
            j1 = int(np.argmin(cand))                                  # the first (lowest) index among equals
            delta = cand[j1]
            u[p[used]] += delta
            v[used] -= delta
            minv[free] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while True:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
            if j0 == 0:
                break
    perm = np.zeros(n, np.int64)
    perm[p[1:] - 1] = np.arange(n)
    return perm


def similarity(layers, l, ref, t, pprev, sprev):
    """S [W, W] fp64 of hidden layer l of the draw t against ref; pprev, sprev: the previous layer's permutation and signs (None
    for l = 0).  The terms are added one after another: bias, incoming rows t = 0 .., then (last hidden layer) outgoing k = 0 .."""
    ob, ok, fin, W = layers[l]
    f64 = lambda a: a.astype(np.float64)
    Kr, Kd = f64(ref[ok:ok + fin * W]).reshape(fin, W), f64(t[ok:ok + fin * W]).reshape(fin, W)
    if pprev is not None:
        Kd = Kd[pprev] * sprev[:, None]
    with np.errstate(all='ignore'):
        S = f64(ref[ob:ob + W])[:, None] * f64(t[ob:ob + W])[None, :]
        for i in range(fin):
            S = S + Kr[i][:, None] * Kd[i][None, :]
        if l == len(layers) - 2:
            _, ok2, fin2, O = layers[l + 1]
            Or, Od = f64(ref[ok2:ok2 + fin2 * O]).reshape(fin2, O), f64(t[ok2:ok2 + fin2 * O]).reshape(fin2, O)
            for k in range(O):
                S = S + Or[:, k][:, None] * Od[:, k][None, :]
    return S


def align(spec, theta, reference, sign=False, gains=None):
    """theta [M, d] fp32, reference [d] fp32 -> out [M, d] fp32, perm [M, H] int32, sign [M, H] int8, score [M, n_hidden] fp64,
    dropped [M] int32.  ``gains``: a list that receives (m, l, G) of every problem solved."""
    if sign and spec.activation != 'tanh':
        raise ValueError('sign fixing is for tanh only')
    theta, ref = np.asarray(theta, np.float32), np.asarray(reference, np.float32)
    layers = _layers(spec)
    nh = len(layers) - 1
    widths = [w for _, _, _, w in layers[:-1]]
    M, H = theta.shape[0], sum(widths)
    out = np.empty_like(theta)
    perm, sgn = np.zeros((M, H), np.int32), np.ones((M, H), np.int8)
    score, dropped = np.zeros((M, nh)), np.zeros(M, np.int32)
    for m in range(M):
        t = theta[m]
        P, Sg, sc = [], [], []
        for l in range(nh):
            W = widths[l]
            S = similarity(layers, l, ref, t, P[-1] if P else None, Sg[-1] if Sg else None)
            if not np.isfinite(S).all():
                P = None
                break
            G = np.abs(S) if sign else S
            if gains is not None:
                gains.append((m, l, G))
            p = hungarian(-G)
            hit = S[np.arange(W), p]
            s = np.where(hit < 0, -1.0, 1.0) if sign else np.ones(W)
            total = 0.0
            for g in G[np.arange(W), p]:                               # ascending i
                total = total + g
            P.append(p), Sg.append(s), sc.append(total)
        if P is None:                                                  # a non-finite similarity: the draw is copied
            out[m], score[m], dropped[m] = t, np.nan, 1
            perm[m] = np.concatenate([np.arange(w) for w in widths] + [np.arange(0)])
            continue
        for l, (ob, ok, fin, W) in enumerate(layers):
            B, K = t[ob:ob + W].copy(), t[ok:ok + fin * W].reshape(fin, W).copy()
            if l < nh:
                s32 = Sg[l].astype(np.float32)
                B, K = B[P[l]] * s32, K[:, P[l]] * s32[None, :]
            if l > 0:
                K = K[P[l - 1]] * Sg[l - 1].astype(np.float32)[:, None]
            out[m, ob:ob + W], out[m, ok:ok + fin * W] = B, K.reshape(-1)
        if nh:
            perm[m], sgn[m], score[m] = np.concatenate(P), np.concatenate(Sg), sc
    return out, perm, sgn, score, dropped


@functools.lru_cache(maxsize=None)
def permutation_aligned(sign, rounds=2):
    """The permutation case aligned as ``metrics.align`` does with reference='first': round 1 to draw 0 of chain 0, round r >= 2
    to the fp64 mean of the aligned draws cast to fp32.  (out [C, S, d], perm [C, S, H], sign, score [C, S, n_hidden], dropped
    [C, S], reference [d] of the last round)."""
    theta = permutation_draws()
    C, S, d = theta.shape
    flat = theta.reshape(-1, d)
    ref = flat[0]
    for _ in range(rounds):
        used = ref
        out, perm, sgn, score, dropped = align(permutation_spec(), flat, used, sign)
        ref = out[dropped == 0].astype(np.float64).mean(axis=0).astype(np.float32)
    res = out.reshape(C, S, d), perm.reshape(C, S, -1), sgn.reshape(C, S, -1), score.reshape(C, S, -1), dropped.reshape(C, S), np.array(used)
    for v in res:
        v.setflags(write=False)
    return res
