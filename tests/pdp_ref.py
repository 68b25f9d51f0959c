"""Partial dependence and ICE curves of the FCN ensemble in NumPy: the yardstick of mile_predict_partial_dependence and of
metrics.partial_dependence_dense.  Everything in fp64 unless ``dtype`` says otherwise; the float32 variant of the forward exists
only to size tolerances (the statistics of its values are still formed in fp64).

h[s, n, i, g, p]: head column p (regression: mu and log sigma, raw; classification: the softmax probabilities with the maximum
taken off) of draw s on row n with x_{n, features[i]} replaced by grid[i][g].
  form='substitute'  writes the grid value into the column and runs oracle.mclmc_oracle.mlp_forward
  form='update'      the library's arithmetic, which is the definition: z_0 = x W_0 + b_0 once, z_0' = z_0 + (v - x_f) W_0[f, :]
The two agree to rounding on finite inputs.  They differ on a row with a non-finite input in column f: substitution takes it out
of the row, the update leaves it in z_0 (inf + (v - inf) w is NaN), so under the definition such a row is dropped for every
feature, f included.
A (draw, row, feature) triple is kept iff all G * P values of the feature are finite."""
import numpy as np

from oracle import mclmc_oracle as O


def _head(ospec, raw):
    if ospec.task == 'regr':
        return raw
    e = np.exp(raw - raw.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def values(ospec, theta, X, features, grid, dtype=np.float64, form='update'):
    """theta [M, d], X [N, F], features [Fs], grid [Fs, G] -> h [M, N, Fs, G, P] in ``dtype``."""
    theta, X, grid = np.asarray(theta, dtype=dtype), np.asarray(X, dtype=dtype), np.asarray(grid, dtype=dtype)
    M, N, (Fs, G) = theta.shape[0], X.shape[0], grid.shape
    out = []
    with np.errstate(all='ignore'):
        if form == 'substitute':
            for i, f in enumerate(features):
                cols = []
                for g in range(G):
                    Xs = X.copy()
                    Xs[:, f] = grid[i, g]
                    cols.append(_head(ospec, O.mlp_forward(ospec, theta, Xs)))
                out.append(np.stack(cols, axis=2))                           # [M, N, G, P]
        elif form == 'update':
            layers = O.unravel(ospec, theta)
            W0, b0 = layers[0]
            z0 = X[None] @ W0 + b0[:, None, :]                                # [M, N, w0]
            for i, f in enumerate(features):
                step = (grid[i][None, :] - X[:, f][:, None]).astype(dtype)   # [N, G]: v - x_f
                z = z0[:, :, None, :] + step[None, :, :, None] * W0[:, f, :][:, None, None, :]
                h = z.reshape(M, N * G, -1)
                for li in range(1, len(layers)):
                    W, b = layers[li]
                    h = O._act(ospec.activation, h) @ W + b[:, None, :]
                out.append(_head(ospec, h).reshape(M, N, G, -1))
        else:
            raise ValueError(form)
    return np.stack(out, axis=2).astype(dtype)


def statistics(h, C):
    """Every output of mile_predict_partial_dependence from h [C * S, N, Fs, G, P] (chain c's draws are rows c * S .. (c + 1) * S - 1),
    formed in fp64, the drop rule included, plus ``kept`` [N, Fs] and ``rows`` [C * S, Fs], the integers behind ``dropped`` and
    the curves."""
    M, N, Fs, G, P = h.shape
    S = M // C
    ok = np.isfinite(h).all(axis=(-1, -2))                                   # [M, N, Fs]
    w = ok[..., None, None].astype(np.float64)
    h = np.where(ok[..., None, None], h.astype(np.float64), 0.0)
    k = ok.sum(axis=0)                                                       # [N, Fs]
    kk = k[..., None, None].astype(np.float64)
    kr = ok.sum(axis=1)                                                      # [M, Fs]
    with np.errstate(all='ignore'):
        ice_mean = h.sum(axis=0) / kk
        d = (h - ice_mean) * w
        ice_sd = np.where(kk > 1, np.sqrt((d * d).sum(axis=0) / np.maximum(kk - 1, 1)), np.where(kk > 0, 0.0, np.nan))
        m = h.sum(axis=1) / kr[..., None, None].astype(np.float64)           # [M, Fs, G, P]: NaN without a kept row
        have = kr > 0                                                        # [M, Fs]
        hw = have[..., None, None].astype(np.float64)
        m0 = np.where(have[..., None, None], m, 0.0)
        nd = have.sum(axis=0)[:, None, None].astype(np.float64)              # [Fs, 1, 1]
        pd_mean = m0.sum(axis=0) / nd
        dm = (m0 - pd_mean) * hw
        pd_sd = np.where(nd > 1, np.sqrt((dm * dm).sum(axis=0) / np.maximum(nd - 1, 1)), np.where(nd > 0, 0.0, np.nan))
        cd = have.reshape(C, S, Fs).sum(axis=1)                              # [C, Fs]
        chain_pd = m0.reshape(C, S, Fs, G, P).sum(axis=1) / cd[..., None, None].astype(np.float64)
    return {'ice_mean': ice_mean, 'ice_sd': ice_sd, 'dropped': (M - k).astype(np.int32), 'curves': m, 'pd_mean': pd_mean, 'pd_sd': pd_sd,
            'chain_pd': chain_pd, 'chain_draws': cd.astype(np.int64), 'kept': k.astype(np.int64), 'rows': kr.astype(np.int64)}


def partial_dependence(ospec, theta, X, features, grid, C, dtype=np.float64, form='update'):
    """``statistics`` of ``values``: theta [C * S, d] -> the dict of mile_predict_partial_dependence."""
    return statistics(values(ospec, theta, X, features, grid, dtype, form), C)
