"""NumPy restatement of the canonical hidden-unit ordering of FCN draws (mile_canonicalize_fcn, include/mile_hip.h), straight
from the rule and from ModelSpec.leaves() offsets.  No torch.

Hidden layers l = 0 .. n_layers - 2 (widths W_l) own [o_l, o_l + W_l) of the H axis.  sign (tanh only): s = -1 iff bias < 0
(-0.0, +0.0 and NaN stay).  key 'bias': s * bias as fp32; 'norm': bias^2 + sum_i kernel[i][j]^2 in fp64, the terms added one
after another, bias first, then i ascending.  Order: ascending key, ties in index order, NaN after every number."""
from __future__ import annotations

import functools

import numpy as np

from tests import fdiag_ref as F

KEYS = ('bias', 'norm')
COMBOS = tuple((k, s) for k in KEYS for s in (False, True))           # the four rule combinations (sign: tanh only)


# The shapes of the tests: the smallest at which each part can go wrong.  name: (in_features, hidden_structure, activation, task, M)
CASES = {
    'perm': (3, F.PERM_WIDTHS, 'tanh', 'regr', F.PERM_C * F.PERM_S),  # the permutation case (its own draws)
    'w64x3': (5, (64, 64, 64, 2), 'relu', 'regr', 7),                 # a full wave per layer, three chained row / column permutations
    'deep12': (4, (3,) * 11 + (2,), 'tanh', 'regr', 5),               # twelve layers: layer10 and layer11 lie before layer2
    'width1': (2, (1, 2), 'tanh', 'regr', 4),                         # nothing to order
    'nohidden': (6, (3,), 'relu', 'classification', 4),               # H = 0: a copy
    'wide': (9, (256, 130, 7), 'sigmoid', 'classification', 3),       # widths above a wave, not a power of two, 147 KB a draw
    'tiled': (54, (256, 256, 7), 'relu', 'classification', 2),        # 326 KB a draw: the row-tiled form
}


def case_spec(name):
    from mile_amd import ModelSpec
    fin, hs, act, task, _ = CASES[name]
    return ModelSpec(fin, hs, activation=act, task=task)


def case_combos(name):
    return tuple((k, s) for k, s in COMBOS if not s or CASES[name][2] == 'tanh')


@functools.lru_cache(maxsize=None)
def case_draws(name):
    """The case's draws [M, d] fp32 (computed once, never changed)."""
    if name == 'perm':
        theta = permutation_draws().reshape(-1, permutation_draws().shape[-1])
    else:
        theta = random_draws(case_spec(name), CASES[name][4], seed=sorted(CASES).index(name) + 10)
        theta.setflags(write=False)
    return theta


@functools.lru_cache(maxsize=None)
def case_canonical(name, key, sign):
    res = canonicalize(case_spec(name), case_draws(name), key, sign)
    for v in res:
        v.setflags(write=False)
    return res


def specials():
    """[3 -> 8 -> 8 -> 2] tanh, 4 draws with hand-placed values: draw 0 has two identical units in layer 0 (units 2 and 5) and
    biases -0.0 / +0.0 in layer 1; draw 1 has +-inf biases; draw 2 a NaN bias; draw 3 is plain."""
    spec = permutation_spec()
    off = {n.split('.', 1)[1]: (o, tuple(sh)) for n, o, sh in spec.leaves()}
    theta = random_draws(spec, 4, seed=77)
    (b0, _), (k0, (fin0, w0)) = off['layer0.bias'], off['layer0.kernel']
    (b1, _), (k1, (fin1, w1)) = off['layer1.bias'], off['layer1.kernel']
    t = theta[0]
    t[b0 + 5] = t[b0 + 2]
    t[k0:k0 + fin0 * w0].reshape(fin0, w0)[:, 5] = t[k0:k0 + fin0 * w0].reshape(fin0, w0)[:, 2]
    t[b1 + 1], t[b1 + 6], t[b1 + 3] = -0.0, 0.0, -0.0
    theta[1][b0 + 4], theta[1][b0 + 1], theta[1][b1 + 7] = np.inf, -np.inf, np.inf
    theta[2][b0 + 3] = np.nan
    theta[2][b1 + 0] = np.nan
    theta[2][b1 + 5] = np.nan
    return spec, theta


def _layers(spec):
    """[(bias offset, kernel offset, fin, fout)] in layer order, from the project's own leaf table."""
    off = {n.split('.', 1)[1]: (o, tuple(sh)) for n, o, sh in spec.leaves()}
    out = []
    for li in range(len(spec.hidden_structure)):
        (ob, (fout,)), (ok, (fin, fo)) = off[f'layer{li}.bias'], off[f'layer{li}.kernel']
        assert fo == fout
        out.append((ob, ok, fin, fout))
    return out


def keys_of(spec, theta, key='bias', sign=False):
    """theta [M, d] fp32 -> [(key [M, W_l], s [M, W_l] fp32)] per hidden layer."""
    if sign and spec.activation != 'tanh':
        raise ValueError('sign fixing is for tanh only')
    theta = np.asarray(theta, np.float32)
    M = theta.shape[0]
    res = []
    for ob, ok, fin, fout in _layers(spec)[:-1]:
        b = theta[:, ob:ob + fout]
        s = np.where(b < 0, np.float32(-1), np.float32(1)).astype(np.float32) if sign else np.ones_like(b)
        if key == 'bias':
            k = (s * b).astype(np.float32)
        elif key == 'norm':
            K = theta[:, ok:ok + fin * fout].reshape(M, fin, fout).astype(np.float64)
            k = b.astype(np.float64) * b.astype(np.float64)
            with np.errstate(all='ignore'):
                for i in range(fin):
                    k = k + K[:, i, :] * K[:, i, :]
        else:
            raise ValueError(key)
        res.append((k, s))
    return res


def canonicalize(spec, theta, key='bias', sign=False):
    """theta [M, d] fp32 -> out [M, d] fp32, perm [M, H] int32, sign [M, H] int8."""
    theta = np.asarray(theta, np.float32)
    M = theta.shape[0]
    layers = _layers(spec)
    perms, signs = [], []
    for k, s in keys_of(spec, theta, key, sign):
        p = np.argsort(k, axis=1, kind='stable')                      # stable; NaNs last, among themselves in index order
        perms.append(p)
        signs.append(np.take_along_axis(s, p, axis=1))
    out = np.empty_like(theta)
    with np.errstate(all='ignore'):
        for li, (ob, ok, fin, fout) in enumerate(layers):
            B = theta[:, ob:ob + fout]
            K = theta[:, ok:ok + fin * fout].reshape(M, fin, fout)
            if li < len(layers) - 1:
                B = np.take_along_axis(B, perms[li], axis=1) * signs[li]
                K = np.take_along_axis(K, perms[li][:, None, :], axis=2) * signs[li][:, None, :]
            if li > 0:
                K = np.take_along_axis(K, perms[li - 1][:, :, None], axis=1) * signs[li - 1][:, :, None]
            out[:, ob:ob + fout] = B
            out[:, ok:ok + fin * fout] = K.reshape(M, fin * fout)
    cat = lambda a, dt: (np.concatenate(a, axis=1) if a else np.zeros((M, 0))).astype(dt)
    return out, cat(perms, np.int32), cat(signs, np.int8)


def orbit_member(spec, theta, seed, flips=False):
    """Another member of every draw's orbit: a random permutation of each hidden layer's units per draw (and, with ``flips``, a
    random sign flip per unit: tanh only).  theta [M, d] fp32 -> [M, d] fp32, every float moved, possibly negated."""
    theta = np.asarray(theta, np.float32)
    rng = np.random.default_rng(seed)
    M = theta.shape[0]
    layers = _layers(spec)
    P = [np.argsort(rng.random((M, fout)), axis=1) for _, _, _, fout in layers[:-1]]
    S = [(rng.integers(0, 2, (M, fout)) * 2 - 1).astype(np.float32) if flips else np.ones((M, fout), np.float32)
         for _, _, _, fout in layers[:-1]]
    out = np.empty_like(theta)
    for li, (ob, ok, fin, fout) in enumerate(layers):
        B = theta[:, ob:ob + fout]
        K = theta[:, ok:ok + fin * fout].reshape(M, fin, fout)
        if li < len(layers) - 1:
            B = np.take_along_axis(B, P[li], axis=1) * S[li]
            K = np.take_along_axis(K, P[li][:, None, :], axis=2) * S[li][:, None, :]
        if li > 0:
            K = np.take_along_axis(K, P[li - 1][:, :, None], axis=1) * S[li - 1][:, :, None]
        out[:, ob:ob + fout] = B
        out[:, ok:ok + fin * fout] = K.reshape(M, fin * fout)
    return out


def random_draws(spec, M, seed, scale=0.7):
    return (scale * np.random.default_rng(seed).standard_normal((M, spec.n_params))).astype(np.float32)


def switches(perm, widths):
    """perm [C, S, H] -> int64 [C, n_hidden]: the draws j >= 1 whose order of layer l differs from draw j - 1's."""
    perm = np.asarray(perm)
    out = np.zeros((perm.shape[0], len(widths)), np.int64)
    o = 0
    for l, w in enumerate(widths):
        span = perm[:, :, o:o + w]
        out[:, l] = (span[:, 1:] != span[:, :-1]).any(axis=2).sum(axis=1)
        o += w
    return out


def permutation_spec():
    from mile_amd import ModelSpec
    return ModelSpec(3, F.PERM_WIDTHS, activation='tanh', task='regr')


@functools.lru_cache(maxsize=None)
def permutation_draws():
    """The permutation case of tests/fdiag_ref.py as the fp32 draws [C, S, d] the library gets (computed once, never changed)."""
    spec = permutation_spec()
    theta = F.permutation_case(tuple((n, o, tuple(sh)) for n, o, sh in spec.leaves()))[0].astype(np.float32)
    theta.setflags(write=False)
    return theta


@functools.lru_cache(maxsize=None)
def permutation_canonical(key, sign):
    """(out [C, S, d] fp32, perm [C, S, H], sign [C, S, H]) of the permutation case under one rule combination."""
    theta = permutation_draws()
    C, S, d = theta.shape
    out, perm, sgn = canonicalize(permutation_spec(), theta.reshape(-1, d), key, sign)
    res = out.reshape(C, S, d), perm.reshape(C, S, -1), sgn.reshape(C, S, -1)
    for v in res:
        v.setflags(write=False)
    return res
