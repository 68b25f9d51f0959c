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

The gradient functions take `dtype`: float64 is the reference; float32 evaluates the same formulas in float32 throughout (constants
are Python floats, so nothing is promoted), which gives the rounding error a float32 implementation of these formulas has
before any change of summation order (tests/leafcheck.py's bound for a leaf that does not meet its fixed tolerance).
"""
from __future__ import annotations

import math

import numpy as np

SQ2PI = math.sqrt(2.0 / math.pi)
MUTANTS = ('zero_qk_kernels', 'dq_unscaled', 'ds_unmasked')     # wrong gradients for tests/test_leafcheck_host.py


def unpack(spec, theta, dtype=np.float64):
    th = np.asarray(theta, dtype=dtype)
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
    qh = (q / math.sqrt(hd)).reshape(N, T, H, hd).transpose(0, 2, 1, 3)
    kh = k.reshape(N, T, H, hd).transpose(0, 2, 1, 3)
    vh = v.reshape(N, T, H, hd).transpose(0, 2, 1, 3)
    s = qh @ kh.transpose(0, 1, 3, 2)                                # [N, H, T, T]
    tokm = x != 0
    mask = (tokm[:, :, None] & tokm[:, None, :])[:, None]
    s = np.where(mask, s, e.dtype.type(np.finfo(np.float32).min))
    raw = s
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
    return dict(e=e, s=raw, q=qh, k=kh, v=vh, p=p, mask=mask, oc=oc, zs=zs, gs=gs, logits=logits, Wq=Wq, Wk=Wk, Wv=Wv, Wo=Wo,
                hd=hd, tokm=tokm)


def pointwise_loglik(spec, theta, x, y):
    """log p(y_n | x_n, theta) [N]."""
    P = unpack(spec, theta)
    f = _forward(spec, P, np.asarray(x, dtype=np.int64))
    lg = f['logits']
    m = lg.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(lg - m).sum(axis=1, keepdims=True)))[:, 0]
    return lg[np.arange(len(lg)), np.asarray(y, dtype=np.int64)] - lse


def attention_backward(f, do, mutant=None):
    """d(q, k, v) [N, T, D] (before the Dense layers) from d(o) [N, H, T, hd] and the forward's intermediates.  `mutant` builds
    one of the wrong gradients of MUTANTS (the 1/sqrt(hd) of dq left out, the mask on ds left out)."""
    assert mutant is None or mutant in MUTANTS, mutant
    p, vh, qh, kh, hd = f['p'], f['v'], f['q'], f['k'], f['hd']
    N, H, T, _ = p.shape
    dv = p.transpose(0, 1, 3, 2) @ do
    dp = do @ vh.transpose(0, 1, 3, 2)
    ds = p * (dp - (dp * p).sum(-1, keepdims=True))
    if mutant != 'ds_unmasked':
        ds = np.where(f['mask'], ds, 0.0)                           # where() drops the masked entries' gradient
    dq = ds @ kh
    if mutant != 'dq_unscaled':
        dq = dq / math.sqrt(hd)
    dk = ds.transpose(0, 1, 3, 2) @ qh
    merge = lambda t: t.transpose(0, 2, 1, 3).reshape(N, T, H * hd)      # noqa: E731
    return merge(dq), merge(dk), merge(dv)


def loglik_and_grad(spec, theta, x, y, dtype=np.float64, mutant=None):
    """sum_n log p(y_n | x_n, theta) and its gradient (flat, spec.leaves() order)."""
    x = np.asarray(x, dtype=np.int64)
    y = np.asarray(y, dtype=np.int64)
    P = unpack(spec, theta, dtype)
    f = _forward(spec, P, x)
    N, T = x.shape
    C, H, D, hd = spec.emb_size, spec.n_heads, spec.qkv_dim, f['hd']
    b = spec.use_bias
    lg = f['logits']
    m = lg.max(axis=1, keepdims=True)
    sm = np.exp(lg - m)
    den = sm.sum(axis=1, keepdims=True)
    ll = float(np.sum((lg - m - np.log(den))[np.arange(N), y]))     # log-softmax, not log(softmax): a label 104 below the row maximum is exp() = 0 in float32
    sm /= den
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
    dq, dk, dv = attention_backward(f, doc.reshape(N, T, H, hd).transpose(0, 2, 1, 3), mutant)
    e = f['e']
    for name, dX, W in (('query', dq, f['Wq']), ('key', dk, f['Wk']), ('value', dv, f['Wv'])):
        G[f'MDPA.{name}.kernel'] = np.einsum('ntc,ntd->cd', e, dX).reshape(C, H, hd)
        if b:
            G[f'MDPA.{name}.bias'] = dX.sum((0, 1)).reshape(H, hd)
    de = dq @ f['Wq'].T + dk @ f['Wk'].T + dv @ f['Wv'].T            # [N, T, C]
    np.add.at(G['TokenEmbedding_0.Embedding.embedding'], x.reshape(-1), de.reshape(-1, C))
    G['TokenEmbedding_0.PositionEmbedding.embedding'] = de.sum(0)
    if mutant == 'zero_qk_kernels':
        G['MDPA.query.kernel'][:] = 0
        G['MDPA.key.kernel'][:] = 0
    flat = np.concatenate([G[n].reshape(-1) for n, _, _ in spec.leaves()])
    assert flat.dtype == np.dtype(dtype) and f['p'].dtype == flat.dtype and lg.dtype == flat.dtype
    return ll, flat


def loglik_grad(spec, theta, x, y, dtype=np.float64, mutant=None):
    """The likelihood's gradient alone for an ensemble: theta [E, d] -> [E, d]."""
    return np.stack([loglik_and_grad(spec, t, x, y, dtype, mutant)[1] for t in np.asarray(theta)])


def logpost_and_grad(spec, theta, x, y, dtype=np.float64, mutant=None):
    """log_unnormalized_posterior and its gradient for an ensemble: theta [E, d] -> (logp [E], grad [E, d])."""
    from oracle import mclmc_oracle as M
    theta = np.asarray(theta, dtype=dtype)
    lls, gs = zip(*(loglik_and_grad(spec, t, x, y, dtype, mutant) for t in theta))
    lp, gp = M.log_prior(spec, theta)
    return np.asarray(lls, dtype=dtype) + lp, np.stack(gs) + gp


def attention_stats(spec, P, x):
    """What makes a problem exercise the softmax, from the forward alone: the median over real query rows and heads of the largest
    attention weight, the smallest weight of an unmasked entry relative to its row's largest, and the largest |logit|."""
    f = _forward(spec, P, np.asarray(x, dtype=np.int64))
    p, m = f['p'], f['mask']
    real = np.broadcast_to(f['tokm'][:, None, :], p.shape[:3])
    top = p.max(axis=-1)
    rel = np.where(np.broadcast_to(m, p.shape), p / top[..., None], 1.0)
    return {'median_top': float(np.median(top[real])), 'min_rel': float(rel.min()),
            'max_logit': float(np.abs(np.where(np.broadcast_to(m, p.shape), f['s'], 0.0)).max())}


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


def sharp_problem(spec, N: int, E: int, seed: int = 0, qk_scale: float | None = None) -> dict:
    """synthetic_problem's rows, labels and parameters with the query and key kernels scaled up so that attention is sharp: the
    softmax's max-subtraction, the 1/sqrt(hd) scale and the softmax backward carry the gradient, which synthetic_problem's
    near-uniform weights (scores of size 2 / C) do not ask of them.  With embeddings of variance 1 / C per entry (token + position:
    |e|^2 = 2) and lecun-normal kernels, a score q.k / sqrt(hd) has standard deviation 2 a^2 / C under a scale a on both kernels,
    whatever hd is; the default a = sqrt(2 C) puts it at 4.  Meant for a wide prior (`prior_scale` large), so that every leaf's
    gradient is the likelihood's."""
    prob = synthetic_problem(spec, N, E, seed)
    a = math.sqrt(2.0 * spec.emb_size) if qk_scale is None else float(qk_scale)
    for n, o, sh in spec.leaves():
        if n.endswith(('MDPA.query.kernel', 'MDPA.key.kernel')):
            prob['theta0'][:, o:o + int(np.prod(sh))] *= np.float32(a)
    prob['qk_scale'] = a
    return prob
