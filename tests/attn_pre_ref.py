"""fp64 NumPy restatement of the PretrainedAttentionClassifier log-likelihood and its gradient
(src/models/text/attention_classifier.py:74-132).  Everything up to the projections is tests/attn_ref.py's AttentionClassifier
(its `_forward` reads the tables from the parameter dict, so the frozen tables go in under the same names); then:

- one more gelu (tanh approximation) after the projection loop, before the classifier;
- no gradient for the tables: they are not parameters (PretrainedAttentionSpec.leaves() has no TokenEmbedding_0 leaves).
"""
from __future__ import annotations

import numpy as np

from tests import attn_ref as A

EMB = 'TokenEmbedding_0.Embedding.embedding'
POS = 'TokenEmbedding_0.PositionEmbedding.embedding'


def params(spec, theta, emb, pos, dtype=np.float64):
    P = A.unpack(spec, theta, dtype)
    P[EMB] = np.asarray(emb, dtype=dtype)
    P[POS] = np.asarray(pos, dtype=dtype)[:spec.context_len]
    return P


def forward(spec, P, x):
    """attn_ref's forward, then the extra gelu and the classifier: f['zf'], f['gf'] (its derivative), f['logits']."""
    f = A._forward(spec, P, np.asarray(x, dtype=np.int64))
    zf, gf = A._gelu(f['zs'][-1])
    f.update(zf=zf, gf=gf, logits=zf @ P['classifier.kernel'] + (P['classifier.bias'] if spec.use_bias else 0.0))
    return f


def _log_softmax(lg):
    m = lg.max(axis=1, keepdims=True)
    return lg - (m + np.log(np.exp(lg - m).sum(axis=1, keepdims=True)))


def pointwise_loglik(spec, theta, emb, pos, x, y):
    """log p(y_n | x_n, theta) [N]."""
    lsm = _log_softmax(forward(spec, params(spec, theta, emb, pos), x)['logits'])
    return lsm[np.arange(len(lsm)), np.asarray(y, dtype=np.int64)]


def loglik_and_grad(spec, theta, emb, pos, x, y, dtype=np.float64, mutant=None):
    """sum_n log p(y_n | x_n, theta) and its gradient (flat, spec.leaves() order); `dtype` and `mutant` as in attn_ref."""
    x = np.asarray(x, dtype=np.int64)
    y = np.asarray(y, dtype=np.int64)
    P = params(spec, theta, emb, pos, dtype)
    f = forward(spec, P, x)
    N, T = x.shape
    C, H, D, hd = spec.emb_size, spec.n_heads, spec.qkv_dim, f['hd']
    b = spec.use_bias
    lsm = _log_softmax(f['logits'])
    ll = float(lsm[np.arange(N), y].sum())
    G = {}
    dl = -np.exp(lsm)
    dl[np.arange(N), y] += 1.0
    zs, gs = f['zs'], f['gs']
    G['classifier.kernel'] = f['zf'].T @ dl
    if b:
        G['classifier.bias'] = dl.sum(0)
    dz = (dl @ P['classifier.kernel'].T) * f['gf']                    # through the extra gelu
    for i in reversed(range(len(spec.projection_dim))):
        da = dz * gs[i]
        G[f'projection_{i}.kernel'] = zs[i].T @ da
        if b:
            G[f'projection_{i}.bias'] = da.sum(0)
        dz = da @ P[f'projection_{i}.kernel'].T
    dout = np.repeat(dz[:, None, :] / T, T, axis=1)                  # d(out) [N, T, C]
    G['MDPA.out.kernel'] = np.einsum('ntd,ntc->dc', f['oc'], dout).reshape(P['MDPA.out.kernel'].shape)
    if b:
        G['MDPA.out.bias'] = dout.sum((0, 1))
    do = (dout @ f['Wo'].T).reshape(N, T, H, hd).transpose(0, 2, 1, 3)
    dq, dk, dv = A.attention_backward(f, do, mutant)
    for name, dX in (('query', dq), ('key', dk), ('value', dv)):
        G[f'MDPA.{name}.kernel'] = np.einsum('ntc,ntd->cd', f['e'], dX).reshape(C, H, hd)
        if b:
            G[f'MDPA.{name}.bias'] = dX.sum((0, 1)).reshape(H, hd)
    if mutant == 'zero_qk_kernels':
        G['MDPA.query.kernel'][:] = 0
        G['MDPA.key.kernel'][:] = 0
    flat = np.concatenate([G[n].reshape(-1) for n, _, _ in spec.leaves()])
    assert flat.dtype == np.dtype(dtype) and f['p'].dtype == flat.dtype and f['logits'].dtype == flat.dtype
    return ll, flat


def loglik_grad(spec, theta, emb, pos, x, y, dtype=np.float64, mutant=None):
    """The likelihood's gradient alone for an ensemble: theta [E, d] -> [E, d]."""
    return np.stack([loglik_and_grad(spec, t, emb, pos, x, y, dtype, mutant)[1] for t in np.asarray(theta)])


def logpost_and_grad(spec, theta, emb, pos, x, y, dtype=np.float64, mutant=None):
    """log_unnormalized_posterior and its gradient for an ensemble: theta [E, d] -> (logp [E], grad [E, d]).  The prior
    covers the sampled leaves only."""
    from oracle import mclmc_oracle as M
    theta = np.asarray(theta, dtype=dtype)
    lls, gs = zip(*(loglik_and_grad(spec, t, emb, pos, x, y, dtype, mutant) for t in theta))
    lp, gp = M.log_prior(spec, theta)
    return np.asarray(lls, dtype=dtype) + lp, np.stack(gs) + gp


def tables(spec, seed: int = 0, extra_pos_rows: int = 0):
    """nn.Embed-like tables (normal, std 1 / sqrt(C)), fp32; pos may have rows past T (the model uses the first T)."""
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    C = spec.emb_size
    emb = (rng.standard_normal((spec.vocab_size, C)) / np.sqrt(C)).astype(np.float32)
    pos = (rng.standard_normal((spec.context_len + extra_pos_rows, C)) / np.sqrt(C)).astype(np.float32)
    return emb, pos


def synthetic_problem(spec, N: int, E: int, seed: int = 0) -> dict:
    """attn_ref.synthetic_problem's rows, labels and parameters (the sampled leaves), plus the tables."""
    prob = A.synthetic_problem(spec, N, E, seed)
    prob['emb'], prob['pos'] = tables(spec, seed)
    return prob


def sharp_problem(spec, N: int, E: int, seed: int = 0, qk_scale: float | None = None) -> dict:
    """attn_ref.sharp_problem (sharp attention, for a wide prior), plus the tables."""
    prob = A.sharp_problem(spec, N, E, seed, qk_scale)
    prob['emb'], prob['pos'] = tables(spec, seed)
    return prob
