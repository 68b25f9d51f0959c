"""The partition target on the CPU oracle: log_prior(first and last layer) + log_likelihood(full net, the other layers
frozen per chain), and its gradient with respect to the compact vector (the reference's log_unnormalized_posterior_partition,
src/training/trainer.py:613-659, restated on oracle/mclmc_oracle.py).

The layout comes from the oracle's own ``param_slices`` (lexicographic layer order), not from the package under test.
"""
from __future__ import annotations

import numpy as np

from oracle import mclmc_oracle as M


def sampled_layers(ospec):
    n = len(ospec.layer_dims)
    return list(range(n)) if n <= 2 else [0, n - 1]


def segments(ospec):
    """[(begin, end)] of the sampled coordinates in the full row, in full-row order, adjacent leaves merged."""
    ents = M.param_slices(ospec)
    spans = []
    for li in sampled_layers(ospec):
        if ents[li]['bias'] is not None:
            spans.append(tuple(ents[li]['bias']))
        spans.append(tuple(ents[li]['kernel']))
    spans.sort()
    out = []
    for b, e in spans:
        if out and out[-1][1] == b:
            out[-1] = (out[-1][0], e)
        else:
            out.append((b, e))
    return out


def index(ospec):
    """The full-row index of every compact coordinate."""
    return np.concatenate([np.arange(b, e) for b, e in segments(ospec)])


def compact_leaves(ospec):
    """[(name, begin, end)] of the sampled leaves inside the COMPACT vector (for tests/leafcheck.py)."""
    idx = index(ospec)
    pos = {int(f): c for c, f in enumerate(idx)}
    ents = M.param_slices(ospec)
    out = []
    for li in sampled_layers(ospec):
        for kind in ('bias', 'kernel'):
            if ents[li][kind] is None:
                continue
            b, e = ents[li][kind]
            out.append((f'layer{li}.{kind}', pos[b], pos[b] + (e - b)))
    return sorted(out, key=lambda t: t[1])


def partition(ospec, full):
    return np.ascontiguousarray(full[..., index(ospec)])


def merge(ospec, compact, frozen):
    out = np.array(np.broadcast_to(frozen, compact.shape[:-1] + (frozen.shape[-1],)), dtype=compact.dtype)
    out[..., index(ospec)] = compact
    return out


def logdensity_and_grad(ospec, frozen, X, y):
    """compact [E, d_s] -> (logp [E], grad [E, d_s]) in compact's dtype: the callable oracle.mclmc_init / mclmc_step /
    tuner_step take.  Merges with the frozen rows and evaluates the oracle on the full net.  Gradient: the oracle's posterior
    gradient restricted to the segments (a sampled coordinate's prior term is its own).  Value: the oracle's likelihood of
    the full net plus its prior of the sampled coordinates only -- summed directly, not as `full posterior - frozen prior`,
    which in float32 cancels ~1e3 nats of frozen prior against each other and loses the digits the tuner parity checks."""
    idx = index(ospec)

    def f(compact):
        dt = compact.dtype
        full = merge(ospec, compact, frozen.astype(dt))
        Xd, yd = X.astype(dt), (y if y.dtype.kind == 'i' else y.astype(dt))
        _, grad = M.logpost_and_grad(ospec, full, Xd, yd)
        ll, _ = M.pointwise_loglik(ospec, M.mlp_forward(ospec, full, Xd), yd)
        lp, _ = M.log_prior(ospec, compact)
        return (lp + ll.sum(axis=-1)).astype(dt), np.ascontiguousarray(grad[:, idx])

    return f
