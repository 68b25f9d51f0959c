"""Input sensitivities of the FCN ensemble in NumPy: the yardstick of mile_predict_sensitivities and of
metrics.sensitivities_dense.  Everything in fp64 unless ``dtype`` says otherwise; the float32 variant of the Jacobian chain
exists only to size tolerances (the statistics of its Jacobians are still formed in fp64).

a_0 = x, z_l = a_l W_l + b_l, a_{l+1} = phi(z_l) for l < L - 1, raw outputs r = z_{L-1}.  Per draw and row
    Jraw[o][f] = d r_o / d x_f = [W_0 diag phi'(z_0) W_1 ... diag phi'(z_{L-2}) W_{L-1}]_{f,o},
phi' as oracle.mclmc_oracle._act_grad has it (relu' = 1 iff z > 0).  Reported columns J[p][f]: regression J = Jraw (mu and
log sigma); classification J[k][f] = pi_k (Jraw[k][f] - sum_j pi_j Jraw[j][f]), pi = softmax(r) with the maximum taken off.
A (draw, row) pair is kept iff its raw outputs and all P * F entries are finite."""
import numpy as np

from oracle import mclmc_oracle as O


def jacobians(ospec, theta, X, dtype=np.float64):
    """theta [M, d], X [N, F] -> (raw [M, N, O], J [M, N, P, F], hidden pre-activations [z_0 .. z_{L-2}], each [M, N, width]) in
    ``dtype``: the backward chain delta_l = (delta_{l+1} W_l^T) * phi'(z_l) from the unit vectors of the outputs."""
    theta, X = np.asarray(theta, dtype=dtype), np.asarray(X, dtype=dtype)
    layers = O.unravel(ospec, theta)
    with np.errstate(all='ignore'):
        raw, zs, hs = O.mlp_forward(ospec, theta, X, keep=True)
        gt = np.swapaxes(layers[-1][0], 1, 2)                                    # [M, P, width]: d r_p / d a_{L-1}, the same on every row
        g = np.broadcast_to(gt[:, None], (theta.shape[0], X.shape[0]) + gt.shape[1:]).copy()
        for l in range(len(layers) - 2, -1, -1):
            dz = g * O._act_grad(ospec.activation, zs[l], hs[l + 1])[:, :, None, :]
            g = np.matmul(dz, np.swapaxes(layers[l][0], 1, 2)[:, None])
        if ospec.task != 'regr':
            m = raw.max(axis=-1, keepdims=True)
            e = np.exp(raw - m)
            pi = e / e.sum(axis=-1, keepdims=True)
            g = pi[..., None] * (g - (pi[..., None] * g).sum(axis=2, keepdims=True))
    return raw.astype(dtype), g.astype(dtype), zs[:-1]


def kept_pairs(raw, J):
    """[M, N] bool: the raw outputs and all P * F entries finite."""
    return np.isfinite(raw).all(axis=-1) & np.isfinite(J).all(axis=(-1, -2))


def statistics(raw, J, C):
    """The seven outputs from raw [C * S, N, O] and J [C * S, N, P, F] (chain c's draws are rows c * S .. (c + 1) * S - 1), formed in
    fp64, plus ``count_pos`` [N, P, F] and ``kept`` [N], the integers behind ``pos`` and ``dropped``."""
    M, N, P, F = J.shape
    S = M // C
    ok = kept_pairs(raw, J)
    J = np.where(ok[..., None, None], J.astype(np.float64), 0.0)
    w = ok[..., None, None].astype(np.float64)
    k = ok.sum(axis=0)
    kk = k[:, None, None].astype(np.float64)
    with np.errstate(all='ignore'):
        mean = J.sum(axis=0) / kk
        d = (J - mean) * w
        M2 = (d * d).sum(axis=0)
        sd = np.where(kk > 1, np.sqrt(M2 / np.maximum(kk - 1, 1)), np.where(kk > 0, 0.0, np.nan))
        cnt = ((J > 0) * w).sum(axis=0)
        Jc, okc = J.reshape(C, S, N, P, F), ok.reshape(C, S, N)
        ck = okc.sum(axis=(1, 2))
        ckk = ck[:, None, None].astype(np.float64)
        ape = Jc.sum(axis=(1, 2)) / ckk
        ab = np.abs(Jc).sum(axis=(1, 2)) / ckk
        pos = cnt / kk
    return {'mean': mean, 'sd': sd, 'pos': pos, 'dropped': (M - k).astype(np.int32), 'chain_ape': ape, 'chain_abs': ab,
            'chain_kept': ck.astype(np.int64), 'count_pos': cnt.astype(np.int64), 'kept': k.astype(np.int64)}


def sensitivities(ospec, theta, X, C, dtype=np.float64):
    """``statistics`` of ``jacobians``: theta [C * S, d] -> the dict of mile_predict_sensitivities."""
    raw, J, _ = jacobians(ospec, theta, X, dtype)
    return statistics(raw, J, C)


def relu_rows_near_zero(ospec, theta, X, rel=4e-6):
    """[N] bool: rows on which some draw has a hidden pre-activation within rounding of 0,
    |z_j| < rel * (sum_i |a_i W_ij| + |b_j|).  There the ReLU mask of an fp32 forward may differ from the fp64 one, and the row's
    Jacobian with it."""
    theta, X = np.asarray(theta, dtype=np.float64), np.asarray(X, dtype=np.float64)
    layers = O.unravel(ospec, theta)
    _, zs, hs = O.mlp_forward(ospec, theta, X, keep=True)
    near = np.zeros(X.shape[0], dtype=bool)
    for l in range(len(layers) - 1):
        W, b = layers[l]
        mag = np.matmul(np.abs(hs[l]), np.abs(W)) + np.abs(b)[:, None, :]
        near |= (np.abs(zs[l]) < rel * mag).any(axis=(0, 2))
    return near


def finite_difference(ospec, theta, X, h=1e-5):
    """J by central differences of the head outputs (mu and log sigma, or the softmax probabilities) in fp64: [M, N, P, F]."""
    theta, X = np.asarray(theta, dtype=np.float64), np.asarray(X, dtype=np.float64)

    def head(x):
        raw = O.mlp_forward(ospec, theta, x)
        if ospec.task == 'regr':
            return raw
        e = np.exp(raw - raw.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)

    cols = []
    for f in range(X.shape[1]):
        step = np.zeros_like(X)
        step[:, f] = h
        cols.append((head(X + step) - head(X - step)) / (2 * h))
    return np.stack(cols, axis=-1)
