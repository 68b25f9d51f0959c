"""fp64 NumPy restatement of the AttentionClassifier log-likelihood and its gradient
(src/models/text/attention_classifier.py on flax 0.8.5; flax is not installed here, so these semantics are
recalled and pinned as choices):

- mask[b] = outer(x[b] != 0, x[b] != 0): by token id, so a 0 in mid-sequence is masked as query and as key.
- e = Embedding[x] + PositionEmbedding[arange(T)]; pad positions are embedded like any other token.
- MultiHeadDotProductAttention: q, k, v = DenseGeneral(C -> [H, hd]); q /= sqrt(hd); s = q . k per head;
  s = where(mask, s, finfo(float32).min); softmax over the keys.  A pad query row is all masked, so its weights are
  uniform 1/T over all T keys and `where` passes it no gradient to q or k (it still passes gradient to every v);
  pad keys of a real query row get weight exactly 0.
- out = DenseGeneral([H, hd] -> C); mean over all T positions (pads included).
- per projection: Dense then gelu (tanh approximation); classifier Dense(n_classes); categorical log-likelihood.
Parameters are the flat vector of AttentionSpec.leaves().
"""
from __future__ import annotations

import numpy as np

SQ2PI = np.sqrt(2.0 / np.pi)


def unpack(spec, theta):
    th = np.asarray(theta, dtype=np.float64)
    return {n: th[o:o + int(np.prod(s))].reshape(s) for n, o, s in spec.leaves()}


def _gelu(a):
    t = np.tanh(SQ2PI * (a + 0.044715 * a ** 3))
    return 0.5 * a * (1.0 + t), 0.5 * (1.0 + t) + 0.5 * a * (1.0 - t * t) * SQ2PI * (1.0 + 3 * 0.044715 * a * a)


def attn_probs(spec, P, x):
    """Attention weights [N, H, T, T] (for the masking checks)."""
    return _forward(spec, P, np.asarray(x, dtype=np.int64))['p']


def _forward(spec, P, x):
    N, T = x.shape
    C, H, D = spec.emb_size, spec.n_heads, spec.qkv_dim
    hd = D // H
    b = spec.use_bias
    e = P['TokenEmbedding_0.Embedding.embedding'][x] + P['TokenEmbedding_0.PositionEmbedding.embedding'][None, :T]
    Wq = P['MDPA.query.kernel'].reshape(C, D)
    Wk = P['MDPA.key.kernel'].reshape(C, D)
    Wv = P['MDPA.value.kernel'].reshape(C, D)
    q = e @ Wq + (P['MDPA.query.bias'].reshape(D) if b else 0.0)
    k = e @ Wk + (P['MDPA.key.bias'].reshape(D) if b else 0.0)
    v = e @ Wv + (P['MDPA.value.bias'].reshape(D) if b else 0.0)
    qh = (q / np.sqrt(hd)).reshape(N, T, H, hd).transpose(0, 2, 1, 3)
    kh = k.reshape(N, T, H, hd).transpose(0, 2, 1, 3)
    vh = v.reshape(N, T, H, hd).transpose(0, 2, 1, 3)
    s = qh @ kh.transpose(0, 1, 3, 2)                                # [N, H, T, T]
    tokm = x != 0
    mask = (tokm[:, :, None] & tokm[:, None, :])[:, None]
    s = np.where(mask, s, np.finfo(np.float32).min)
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    o = p @ vh                                                        # [N, H, T, hd]
    oc = o.transpose(0, 2, 1, 3).reshape(N, T, D)
    Wo = P['MDPA.out.kernel'].reshape(D, C)
    out = oc @ Wo + (P['MDPA.out.bias'] if b else 0.0)
    z = out.mean(axis=1)
    zs, gs = [z], []
    for i in range(len(spec.projection_dim)):
        a = z @ P[f'projection_{i}.kernel'] + (P[f'projection_{i}.bias'] if b else 0.0)
        z, gp = _gelu(a)
        zs.append(z)
        gs.append(gp)
    logits = z @ P['classifier.kernel'] + (P['classifier.bias'] if b else 0.0)
    return dict(e=e, q=qh, k=kh, v=vh, p=p, mask=mask, oc=oc, zs=zs, gs=gs, logits=logits, Wq=Wq, Wk=Wk, Wv=Wv, Wo=Wo,
                hd=hd, tokm=tokm)


def pointwise_loglik(spec, theta, x, y):
    """log p(y_n | x_n, theta) [N]."""
    P = unpack(spec, theta)
    f = _forward(spec, P, np.asarray(x, dtype=np.int64))
    lg = f['logits']
    m = lg.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(lg - m).sum(axis=1, keepdims=True)))[:, 0]
    return lg[np.arange(len(lg)), np.asarray(y, dtype=np.int64)] - lse


def loglik_and_grad(spec, theta, x, y):
    """sum_n log p(y_n | x_n, theta) and its gradient (flat, spec.leaves() order)."""
    x = np.asarray(x, dtype=np.int64)
    y = np.asarray(y, dtype=np.int64)
    P = unpack(spec, theta)
    f = _forward(spec, P, x)
    N, T = x.shape
    C, H, D, hd = spec.emb_size, spec.n_heads, spec.qkv_dim, f['hd']
    b = spec.use_bias
    lg = f['logits']
    m = lg.max(axis=1, keepdims=True)
    sm = np.exp(lg - m)
    sm /= sm.sum(axis=1, keepdims=True)
    ll = float(np.sum(np.log(sm[np.arange(N), y])))
    G = {n: np.zeros_like(v) for n, v in P.items()}
    dl = -sm
    dl[np.arange(N), y] += 1.0
    zs, gs = f['zs'], f['gs']
    G['classifier.kernel'] = zs[-1].T @ dl
    if b:
        G['classifier.bias'] = dl.sum(0)
    dz = dl @ P['classifier.kernel'].T
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
    doc = dout @ f['Wo'].T                                           # [N, T, D]
    do = doc.reshape(N, T, H, hd).transpose(0, 2, 1, 3)
    p, vh, qh, kh = f['p'], f['v'], f['q'], f['k']
    dv = p.transpose(0, 1, 3, 2) @ do
    dp = do @ vh.transpose(0, 1, 3, 2)
    ds = p * (dp - (dp * p).sum(-1, keepdims=True))
    ds = np.where(f['mask'], ds, 0.0)                               # where() drops the masked entries' gradient
    dq = (ds @ kh) / np.sqrt(hd)
    dk = ds.transpose(0, 1, 3, 2) @ qh
    merge = lambda t: t.transpose(0, 2, 1, 3).reshape(N, T, D)      # noqa: E731
    dq, dk, dv = merge(dq), merge(dk), merge(dv)
    e = f['e']
    for name, dX, W in (('query', dq, f['Wq']), ('key', dk, f['Wk']), ('value', dv, f['Wv'])):
        G[f'MDPA.{name}.kernel'] = np.einsum('ntc,ntd->cd', e, dX).reshape(C, H, hd)
        if b:
            G[f'MDPA.{name}.bias'] = dX.sum((0, 1)).reshape(H, hd)
    de = dq @ f['Wq'].T + dk @ f['Wk'].T + dv @ f['Wv'].T            # [N, T, C]
    np.add.at(G['TokenEmbedding_0.Embedding.embedding'], x.reshape(-1), de.reshape(-1, C))
    G['TokenEmbedding_0.PositionEmbedding.embedding'] = de.sum(0)
    flat = np.concatenate([G[n].reshape(-1) for n, _, _ in spec.leaves()])
    return ll, flat


def logpost_and_grad(spec, theta, x, y):
    """log_unnormalized_posterior and its gradient for an ensemble: theta [E, d] -> (logp [E], grad [E, d])."""
    from oracle import mclmc_oracle as M
    theta = np.asarray(theta, dtype=np.float64)
    lls, gs = zip(*(loglik_and_grad(spec, t, x, y) for t in theta))
    lp, gp = M.log_prior(spec, theta)
    return np.asarray(lls) + lp, np.stack(gs) + gp


def synthetic_problem(spec, N: int, E: int, seed: int = 0) -> dict:
    """Seeded token rows that exercise every masking rule, labels, and small random parameters.  Row 0 repeats one token
    (colliding embedding adds) and holds id V-1; row 1 is fully padded (when N > 1); row 2 has a pad id in mid-sequence."""
    rng = np.random.Generator(np.random.PCG64(seed))
    T, V = spec.context_len, spec.vocab_size
    lengths = rng.integers(1, T + 1, N)
    x = rng.integers(1, V, (N, T))
    x = np.where(np.arange(T)[None] < lengths[:, None], x, 0)
    x[0, :] = 0
    x[0, :max(1, T // 2)] = min(3, V - 1)
    x[0, 0] = V - 1
    if N > 1:
        x[1, :] = 0
    if N > 2 and T > 4:
        x[2, :] = rng.integers(1, V, T)
        x[2, T // 2] = 0
    y = rng.integers(0, spec.n_classes, N).astype(np.int32)
    theta = np.zeros((E, spec.n_params), dtype=np.float32)
    for n, o, sh in spec.leaves():
        k = int(np.prod(sh))
        if n.endswith('embedding'):
            theta[:, o:o + k] = rng.standard_normal((E, k)) / np.sqrt(sh[-1])
        elif n.endswith('kernel'):
            fan = sh[0] * (sh[1] if n.endswith('out.kernel') else 1)
            theta[:, o:o + k] = rng.standard_normal((E, k)) / np.sqrt(fan)
        else:
            theta[:, o:o + k] = 0.05 * rng.standard_normal((E, k))
    d = spec.n_params
    return {'X': x.astype(np.float32), 'x': x, 'y': y, 'theta0': theta, 'u0': rng.standard_normal((E, d)).astype(np.float32),
            'eps': (1e-3 * (1 + 0.05 * rng.uniform(-1, 1, E))).astype(np.float32),
            'L': (np.sqrt(d) * 1e-2 * (1 + 0.05 * rng.uniform(-1, 1, E))).astype(np.float32)}
