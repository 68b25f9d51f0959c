"""fp64 NumPy restatement of mile_calibration's contract (include/mile_hip.h): ``probs`` maps logits to the group
probabilities, ``decide`` maps group probabilities to every discrete and summed output.  Every sum that decides something --
the softmax denominator, a set's cumulative sum, the Brier score -- runs in the stated order."""
import numpy as np


def probs(raw, C, S):
    """raw [C * S, N, K] float32 -> (P [C + 1, N, K] float64, kept [C + 1, N] int32); the last group is the ensemble."""
    raw = np.asarray(raw)
    _, N, K = raw.shape
    z = raw.reshape(C, S, N, K)
    ok = np.isfinite(z).all(axis=-1)                                   # [C, S, N]
    zd = np.where(ok[..., None], z, np.float32(0.0)).astype(np.float64)   # a dropped draw: any finite stand-in, masked below
    e = np.exp(zd - zd.max(axis=-1, keepdims=True))
    se = np.zeros(e.shape[:-1])
    for k in range(K):                                                 # class order
        se = se + e[..., k]
    p = e / se[..., None]
    sums = np.zeros((C, N, K))
    for j in range(S):                                                 # draw order
        sums = sums + np.where(ok[:, j, :, None], p[:, j], 0.0)
    cnt = ok.sum(axis=1)
    tot = np.zeros((N, K))
    for c in range(C):                                                 # chain order
        tot = tot + sums[c]
    kept = np.concatenate([cnt, cnt.sum(axis=0, keepdims=True)]).astype(np.int32)
    with np.errstate(invalid='ignore', divide='ignore'):
        P = np.concatenate([sums, tot[None]]) / kept[..., None].astype(np.float64)
    P[kept == 0] = np.nan
    return P, kept


def decide(P, kept, y, coverages, n_bins):
    """P [G, N, K] float64, kept [G, N], y [N] int or None -> dict: per group ``order`` [G, N, K], ``set_size`` [G, N, Q],
    ``rank`` [G, N] (int32; the library returns the last group's), ``totals`` [G, 5 + 2 Q], ``bins`` [G, n_bins, 3]."""
    P = np.asarray(P, dtype=np.float64)
    G, N, K = P.shape
    cov = [float(c) for c in coverages]
    Q = len(cov)
    order = np.zeros((G, N, K), dtype=np.int32)
    size = np.zeros((G, N, Q), dtype=np.int32)
    rank = np.zeros((G, N), dtype=np.int32)
    totals = np.zeros((G, 5 + 2 * Q))
    bins = np.zeros((G, n_bins, 3))
    for g in range(G):
        for n in range(N):
            if kept[g, n] == 0:
                order[g, n] = np.arange(K)
                continue
            p = P[g, n]
            o = sorted(range(K), key=lambda k: (-p[k], k))             # P descending, ties to the lower class index
            order[g, n] = o
            cum = 0.0
            for i, k in enumerate(o):                                  # sequential
                cum = cum + p[k]
                for q in range(Q):
                    if size[g, n, q] == 0 and cum >= cov[q]:
                        size[g, n, q] = i + 1
            size[g, n][size[g, n] == 0] = K
            if y is None:
                continue
            yn = int(y[n])
            if yn < 0 or yn >= K:
                totals[g, 4] += 1
                continue
            r = o.index(yn) + 1
            rank[g, n] = r
            brier = 0.0
            for k in range(K):                                         # class order
                d = p[k] - (1.0 if k == yn else 0.0)
                brier = brier + d * d
            conf = p[o[0]]
            with np.errstate(divide='ignore'):
                nll = -np.log(p[yn])
            b = min(n_bins - 1, int(np.floor(conf * n_bins)))
            totals[g, 0] += 1
            totals[g, 1] += r == 1
            totals[g, 2] += brier
            totals[g, 3] += nll
            for q in range(Q):
                totals[g, 5 + q] += r <= size[g, n, q]
                totals[g, 5 + Q + q] += size[g, n, q]
            bins[g, b] += (1.0, conf, float(r == 1))
    return {'order': order, 'set_size': size, 'rank': rank, 'totals': totals, 'bins': bins}
