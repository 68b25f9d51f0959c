"""LPPD, the parity metric (mirror of src/inference/metrics.py:247-312,428-446), and the
batched predictive forward pass that feeds it (src/inference/evaluation.py:16-43 does a Python
loop of module.apply per sample; here all C*S samples go through one batched matmul chain).
Evaluation is a consumer of the hot path, not part of it: plain torch on the device.
"""
from __future__ import annotations

import math

import torch

from mile_amd.spec import ModelSpec

_LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def predict(spec: ModelSpec, flat: torch.Tensor, X: torch.Tensor, batch: int = 256) -> torch.Tensor:
    """flat [..., d] samples -> network outputs [..., N, out] (FullyConnected.__call__)."""
    lead = flat.shape[:-1]
    th = flat.reshape(-1, flat.shape[-1])
    X = X.to(th.device, th.dtype)
    outs = []
    leaves = {n: (o, s) for n, o, s in spec.leaves()}
    act = {'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}[spec.activation]
    nl = len(spec.hidden_structure)
    for b0 in range(0, th.shape[0], batch):
        t = th[b0:b0 + batch]
        h = X[None].expand(t.shape[0], -1, -1)
        for li in range(nl):
            ko, ks = leaves[f'{spec.root}.layer{li}.kernel']
            bo, bs = leaves[f'{spec.root}.layer{li}.bias']
            W = t[:, ko:ko + ks[0] * ks[1]].reshape(-1, *ks)
            b = t[:, bo:bo + bs[0]]
            h = torch.baddbmm(b[:, None, :], h, W)
            if li < nl - 1:
                h = act(h)
        outs.append(h)
    out = torch.cat(outs, dim=0)
    return out.reshape(*lead, *out.shape[1:])


def pointwise_lppd(lvals: torch.Tensor, y: torch.Tensor, task: str) -> torch.Tensor:
    """lvals [C, S, N, out] -> [C, S, N] (metrics.py:247-294)."""
    if lvals.ndim == 3:
        lvals = lvals[None]
    elif lvals.ndim == 2:
        lvals = lvals[None, None]
    y = y.to(lvals.device)
    if task in ('regr', 'regression'):
        sigma = torch.exp(lvals[..., 1]).clamp(min=1e-6, max=1e6)
        r = (y.to(lvals.dtype) - lvals[..., 0]) / sigma
        return -0.5 * r * r - torch.log(sigma) - _LOG_SQRT_2PI
    logp = torch.log_softmax(lvals, dim=-1)
    idx = y.to(torch.int64).expand(lvals.shape[:-1])[..., None]
    return torch.gather(logp, -1, idx)[..., 0]


def lppd(lppd_pointwise: torch.Tensor) -> torch.Tensor:
    """metrics.py:297-312: mean_n( logsumexp_{c,s} l - log(C*S) )."""
    C, S = lppd_pointwise.shape[:2]
    flat = lppd_pointwise.reshape(C * S, -1)
    return (torch.logsumexp(flat, dim=0) - math.log(C * S)).mean()


def running_lppd(lppd_pointwise: torch.Tensor) -> torch.Tensor:
    """metrics.py:428-446: running mean over the sample axis, averaged over obs and chains."""
    e = torch.exp(lppd_pointwise)
    cnt = torch.arange(1, e.shape[1] + 1, device=e.device, dtype=e.dtype)[None, :, None]
    return torch.log(torch.cumsum(e, dim=1) / cnt).mean(dim=-1).mean(dim=0)


def curve_points(S: int, n: int = 64) -> list:
    """Default draw counts of the LPPD-versus-draws curves: all of 1..S when S <= n, otherwise n points spaced
    geometrically from 1 to S (rounded, repeats moved up to the next free integer), 1 and S always among them."""
    S, n = int(S), int(n)
    if S < 1 or n < 1:
        raise ValueError('curve_points: S >= 1 and n >= 1')
    if S <= n:
        return list(range(1, S + 1))
    if n == 1:
        return [S]
    pts, prev = [], 0
    for i in range(n):
        k = max(prev + 1, int(round(S ** (i / (n - 1)))))
        k = min(k, S - (n - 1 - i))                                    # room for the points still to come
        pts.append(k)
        prev = k
    pts[-1] = S
    return pts


def streamed_lppd(engine, samples, x, y, curve_points=None, max_draws_per_pass: int = 0) -> dict:
    """``lppd`` and ``running_lppd`` of samples [C, S, d] on (x, y), the LPPD of each chain and of each row, streamed on the
    device in a stable log-sum-exp form (Engine.lppd_stream / mile_lppd_stream): no [C, S, N] tensor, no -inf from exp(l)
    underflowing.  ``run_chain`` is ``running_lppd`` at the curve points, ``run_ens`` is ``lppd`` of the first k draws of
    every chain, ``lppd`` the figure of all draws."""
    return engine.lppd_stream(samples, x, y, curve_points=curve_points, max_draws_per_pass=max_draws_per_pass)


def rank_normalize_array(samples: torch.Tensor) -> torch.Tensor:
    """metrics.py:226-244: overall ranks (average rank for ties) -> normal quantiles."""
    flat = samples.reshape(-1).to(torch.float64)
    n = flat.numel()
    order = torch.argsort(flat, stable=True)
    sv = flat[order]
    ranks_sorted = torch.arange(1, n + 1, dtype=torch.float64, device=flat.device)
    # average rank within runs of equal values (scipy.stats.rankdata method='average')
    new_run = torch.ones(n, dtype=torch.bool, device=flat.device)
    new_run[1:] = sv[1:] != sv[:-1]
    run_id = torch.cumsum(new_run.to(torch.int64), 0) - 1
    n_runs = int(run_id[-1].item()) + 1 if n else 0
    sums = torch.zeros(n_runs, dtype=torch.float64, device=flat.device).index_add_(0, run_id, ranks_sorted)
    cnts = torch.zeros(n_runs, dtype=torch.float64, device=flat.device).index_add_(0, run_id, torch.ones_like(ranks_sorted))
    ranks = torch.empty_like(flat)
    ranks[order] = (sums / cnts)[run_id]
    tmp = (ranks - 0.375) / (n + 0.25)
    return (math.sqrt(2.0) * torch.erfinv(2.0 * tmp - 1.0)).reshape(samples.shape).to(samples.dtype)


def effective_sample_size(x: torch.Tensor, rank_normalize: bool = True) -> torch.Tensor:
    """metrics.py:386-405: x [C, S, ...] -> per-chain ESS [C, ...].  Each trailing column is rank-normalised over
    the pooled C*S draws, then every chain goes through the single-chain FFT/Geyer estimator (the reference calls
    numpyro's; here the Stan-style estimator of mile_amd.diagnostics, the same one the tuner uses)."""
    from mile_amd.diagnostics import effective_sample_size as ess1
    C, S = x.shape[:2]
    cols = x.reshape(C, S, -1)
    if rank_normalize:
        cols = torch.stack([rank_normalize_array(cols[:, :, k]) for k in range(cols.shape[2])], dim=2)
    out = torch.stack([ess1(cols[c][None]) for c in range(C)])
    return out.reshape(C, *x.shape[2:])


# ---- chain diagnostics (src/inference/metrics.py:354-383, 449-523): plain torch here, which is also what CPU tensors get;
# chain_diagnostics sends CUDA fp32 draws through the library's fused kernels (mile_chain_diagnostics) instead.

def between_chain_var(x: torch.Tensor) -> torch.Tensor:
    """metrics.py:354-367: x [C, S, ...] -> ddof-1 variance of the C chain means (NaN for one chain, as NumPy's)."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return x.mean(dim=1).var(dim=0, unbiased=True)


def within_chain_var(x: torch.Tensor) -> torch.Tensor:
    """metrics.py:370-383: x [C, S, ...] -> mean over chains of the ddof-1 variance over S."""
    return x.var(dim=1, unbiased=True).mean(dim=0)


def rank_normalize_columns(x2: torch.Tensor) -> torch.Tensor:
    """x2 [n, m] -> float64 normal scores of every column ranked over its n entries, average rank for ties (what
    rank_normalize_array gives column by column), from ONE batched sort.  A column with a NaN is NaN throughout."""
    return _scores_of_sorted(*torch.sort(x2.to(torch.float64), dim=0, stable=True))


def _scores_of_sorted(sv: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    """rank_normalize_columns' scores from the stable sort (values, indices) of the columns [n, m], in any float dtype."""
    return _scores_of_sorted_rows(sv.t().contiguous(), order.t().contiguous()).t()


def _scores_of_sorted_rows(sv: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    """The scores of m series laid out as rows [m, n], from their stable sort along dim 1.  The tie groups come from two scans
    along the contiguous axis: a scan down the rows of [n, m] is an order of magnitude slower on the device (59 ms against the
    sort's 4 ms at [128 000, 262]); the integers, and so the scores, are the same either way."""
    n = sv.shape[1]
    pos = torch.arange(n, device=sv.device, dtype=torch.int64)[None, :].expand_as(order)
    first = torch.ones_like(order, dtype=torch.bool)
    first[:, 1:] = sv[:, 1:] != sv[:, :-1]
    last = torch.ones_like(first)
    last[:, :-1] = first[:, 1:]
    lo = torch.cummax(torch.where(first, pos, torch.zeros_like(pos)), dim=1).values
    hi = torch.flip(torch.cummin(torch.flip(torch.where(last, pos, torch.full_like(pos, n)), [1]), dim=1).values, [1])
    ranks = torch.empty_like(sv, dtype=torch.float64).scatter_(1, order, (lo + hi).to(torch.float64) * 0.5 + 1.0)
    z = torch.special.ndtri((ranks - 0.375) / (n + 0.25))
    return torch.where(torch.isnan(sv[:, -1:]).expand_as(z), torch.full_like(z, float('nan')), z)


def _pooled_scores(x: torch.Tensor) -> torch.Tensor:
    """x [C, S, ...] -> float64 scores of every trailing column ranked over its pooled C*S draws."""
    C, S = x.shape[:2]
    return rank_normalize_columns(x.reshape(C * S, -1)).reshape(x.shape)


def gelman_split_r_hat(samples: torch.Tensor, n_splits: int, rank_normalize: bool = True) -> torch.Tensor:
    """metrics.py:449-494: split R-hat over all C * n_splits pieces, samples [C, S, ...] -> [...] (float64)."""
    import warnings
    C, S = samples.shape[:2]
    if S % n_splits:
        raise ValueError('Number of samples must be divisible by n_splits')
    n = S // n_splits
    if n < 50:
        warnings.warn(message='Number of samples should be at least 50x the number of splits', category=UserWarning)
    z = _pooled_scores(samples) if rank_normalize else samples.to(torch.float64)
    splits = z.reshape(C * n_splits, n, *samples.shape[2:])
    wcv, bcv = within_chain_var(splits), between_chain_var(splits)
    return torch.sqrt(((n - 1) / n * wcv + bcv) / wcv)


def split_chain_r_hat(samples: torch.Tensor, n_splits: int, rank_normalize: bool = True) -> torch.Tensor:
    """metrics.py:497-523: gelman_split_r_hat of every chain on its own (ranked within the chain) -> [C, ...]."""
    return torch.stack([gelman_split_r_hat(ch[None], n_splits, rank_normalize) for ch in samples])


LAST_DIAG_PATH = None       # how the last chain_diagnostics call ran: 'torch', 'library' or 'library+torch_sort'


def _library_diagnostics(x: torch.Tensor, n_splits: int) -> dict:
    """x [C, S, d] contiguous CUDA fp32 -> the five statistics from mile_chain_diagnostics.  Past the library's pooled
    bound (C*S > DIAG_POOL_MAX) only the pooled ranking is done here, one batched torch.sort per chunk of columns, and the
    scores go back into the same ESS / R-hat kernels."""
    global LAST_DIAG_PATH
    from mile_amd import _lib
    B = _lib.DIAG_BITS
    C, S, d = x.shape
    new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=x.device)
    out = {'ess': new(C, d), 'crhat': new(C, d), 'rhat': new(d), 'wcv': new(d), 'bcv': new(d)}
    if C * S <= _lib.DIAG_POOL_MAX:
        _diag_call(x, n_splits, B['wcv'] | B['bcv'] | B['ess'] | B['crhat'] | B['rhat'], **out)
        LAST_DIAG_PATH = 'library'
    else:
        _diag_call(x, n_splits, B['wcv'] | B['bcv'] | B['crhat'], wcv=out['wcv'], bcv=out['bcv'], crhat=out['crhat'])
        out['ess'], out['rhat'] = _pooled_ess_rhat(x, n_splits)
        LAST_DIAG_PATH = 'library+torch_sort'
    return out


def _diag_call(src: torch.Tensor, n_splits: int, what: int, **o):
    """mile_chain_diagnostics on src [C, S, m] contiguous CUDA fp32 with a workspace of the size it asks for; o: the output
    tensors of the bits in `what`, by name."""
    import ctypes as Ct
    from mile_amd import _lib
    lib = _lib.load_library()
    C, S, m = src.shape
    ptr = lambda t: Ct.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.device(src.device):
        ws = torch.empty(max(int(lib.mile_chain_diagnostics_workspace(C, S, m, what)), 8), dtype=torch.uint8, device=src.device)
        stream = Ct.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
        _lib.check(lib.mile_chain_diagnostics(ptr(src), C, S, m, n_splits, what, ptr(o.get('wcv')), ptr(o.get('bcv')),
                                              ptr(o.get('ess')), ptr(o.get('crhat')), ptr(o.get('rhat')), ptr(ws), ws.numel(),
                                              stream), lib)


def _pooled_ess_rhat(x: torch.Tensor, n_splits: int):
    """x [C, S, m] CUDA fp32 with C * S past the library's pooled bound -> (ess [C, m], rhat [m]): the pooled ranking by one
    batched torch.sort per chunk of columns, the scores through the library's ESS / R-hat kernels (MILE_DIAG_POOLED_INPUT).
    The one torch-sort path: the parameters (_library_diagnostics) and the function-space columns both come here."""
    from mile_amd._lib import DIAG_BITS as B
    C, S, m = x.shape
    new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=x.device)
    ess, rhat = new(C, m), new(m)
    step = max(1, (1 << 28) // (C * S * 8))                         # columns per sort: the fp64 keys stay under 256 MB
    for k0 in range(0, m, step):
        z = _pooled_scores(x[:, :, k0:k0 + step]).to(torch.float32).contiguous()
        e, r = new(C, z.shape[2]), new(z.shape[2])
        _diag_call(z, n_splits, B['ess'] | B['rhat'] | B['pooled_input'], ess=e, rhat=r)
        ess[:, k0:k0 + step] = e
        rhat[k0:k0 + step] = r
    return ess, rhat


def chain_diagnostics(samples: torch.Tensor, n_splits: int = 2) -> dict:
    """samples [C, S, ...] -> {'ess' [C, ...], 'crhat' [C, ...], 'rhat' [...], 'wcv' [...], 'bcv' [...]}: the reference's
    effective_sample_size, split_chain_r_hat and gelman_split_r_hat (rank-normalised) and within / between chain variance
    of every parameter.  CUDA fp32 draws run in the library's fused kernels (fp32 results); anything else in the torch
    functions above (float64 results) -- CPU tensors, other dtypes, and, with a UserWarning, chains shorter than 4 or
    longer than 4096 draws, which the kernels do not take."""
    global LAST_DIAG_PATH
    import warnings
    C, S = samples.shape[:2]
    if S % n_splits:
        raise ValueError('Number of samples must be divisible by n_splits')
    if S // n_splits < 50:
        warnings.warn(message='Number of samples should be at least 50x the number of splits', category=UserWarning)
    trail = tuple(samples.shape[2:])
    from mile_amd._lib import DIAG_S_MAX, DIAG_S_MIN
    in_range = DIAG_S_MIN <= S <= DIAG_S_MAX
    if samples.is_cuda and samples.dtype == torch.float32 and not in_range:
        warnings.warn(f'chain_diagnostics: {S} draws per chain is outside the range of the HIP kernels '
                      f'[{DIAG_S_MIN}, {DIAG_S_MAX}]; using the torch functions', category=UserWarning)
    if samples.is_cuda and samples.dtype == torch.float32 and in_range:
        res = _library_diagnostics(samples.reshape(C, S, -1).contiguous(), n_splits)
        return {k: v.reshape(*((C,) if k in ('ess', 'crhat') else ()), *trail) for k, v in res.items()}
    from mile_amd.diagnostics import effective_sample_size as ess1
    x = samples.to(torch.float64)
    z = _pooled_scores(x).reshape(C, S, -1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)              # (already raised above, once)
        crhat, rhat = split_chain_r_hat(x, n_splits), gelman_split_r_hat(x, n_splits)
    LAST_DIAG_PATH = 'torch'
    return {'ess': torch.stack([ess1(z[c][None]) for c in range(C)]).reshape(C, *trail), 'crhat': crhat, 'rhat': rhat,
            'wcv': within_chain_var(x), 'bcv': between_chain_var(x)}


# ---- tail diagnostics (Vehtari, Gelman, Simpson, Carpenter & Buerkner 2021): the pooled ESS of the bulk, the tails and the mean,
# the MCSE of the mean and the folded split R-hat.  The definitions are stated once, in include/mile_hip.h
# (mile_chain_diagnostics_tail); the library runs them on CUDA fp32 draws, the dense forms here are the CPU statement and, for
# the series, the path past the library's pooled bound.

LAST_DTAIL_PATH = None      # how the last tail_diagnostics call ran: 'torch', 'library' or 'library+torch_sort'
TAIL_OUTPUTS = ('ess_bulk', 'ess_tail', 'ess_mean', 'mcse_mean', 'rhat_folded')


def tail_quantile_indices(n: int) -> tuple:
    """The integer positions in the n pooled sorted draws: (q_lo, q_hi, lower middle, upper middle)."""
    return (n + 19) // 20 - 1, (19 * n + 19) // 20 - 1, (n - 1) // 2, n // 2


def tail_series_plane(xp: torch.Tensor) -> dict:
    """xp [m, n], every row the n pooled draws of one column -> the derived series as rows [m, n]: 'z', 'zf' (float64 pooled
    normal scores of the draws and of the draws folded about the pooled median), 'i_lo', 'i_hi' (the 0 / 1 of x <= q_lo,
    x <= q_hi, in xp's dtype), and 'quantiles' [3, m] (q_lo, q_hi, the median) in xp's dtype.  Order statistics, the median's
    rounding and the fold are evaluated in xp's dtype, so fp32 draws give the library's fp32 series; a column with a NaN has NaN
    quantiles and scores.  One stable sort of the draws serves the order statistics and the ranks, one more the folded ranks."""
    n = xp.shape[1]
    xs, order = torch.sort(xp, dim=1, stable=True)
    lo, hi, a, b = tail_quantile_indices(n)
    med = ((xs[:, a].to(torch.float64) + xs[:, b].to(torch.float64)) / 2).to(xp.dtype)
    quant = torch.stack([xs[:, lo], xs[:, hi], med])
    quant = torch.where(torch.isnan(xs[:, -1])[None].expand_as(quant), torch.full_like(quant, float('nan')), quant)
    z = _scores_of_sorted_rows(xs, order)
    del xs, order
    f = (xp - quant[2][:, None]).abs()
    zf = _scores_of_sorted_rows(*torch.sort(f, dim=1, stable=True))
    return {'z': z, 'zf': zf, 'i_lo': (xp <= quant[0][:, None]).to(xp.dtype), 'i_hi': (xp <= quant[1][:, None]).to(xp.dtype),
            'quantiles': quant}


def tail_series_dense(x: torch.Tensor) -> dict:
    """x [C, S, m] -> ``tail_series_plane`` of its columns, every series back in x's layout [C, S, m]."""
    C, S, m = x.shape
    ser = tail_series_plane(x.reshape(C * S, m).t().contiguous())
    return {k: (v if k == 'quantiles' else v.t().reshape(C, S, m)) for k, v in ser.items()}


def multichain_ess_dense(v: torch.Tensor, n_splits: int) -> torch.Tensor:
    """v [C, S, m] -> ESS_mc [m]: mile_amd.diagnostics.effective_sample_size on the C * n_splits pieces, NaN where the weighted
    variance is not a positive finite number (a series constant over all pooled draws, a non-finite draw)."""
    import warnings
    from mile_amd.diagnostics import effective_sample_size as ess_mc
    C, S, m = v.shape
    pieces = v.reshape(C * n_splits, S // n_splits, m)
    ess = ess_mc(pieces)
    pc = pieces.to(ess.dtype)
    wv = pc.var(dim=1, unbiased=False).mean(dim=0)
    if pc.shape[0] > 1:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            wv = wv + pc.mean(dim=1).var(dim=0, unbiased=True)
    return torch.where((wv > 0) & torch.isfinite(wv), ess, torch.full_like(ess, float('nan')))


def _split_r_hat_of_scores(z: torch.Tensor, n_splits: int) -> torch.Tensor:
    """gelman_split_r_hat's formula on scores z [C, S, m] that are ranked already."""
    C, S, m = z.shape
    n = S // n_splits
    splits = z.reshape(C * n_splits, n, m)
    wcv = within_chain_var(splits)
    return torch.sqrt(((n - 1) / n * wcv + between_chain_var(splits)) / wcv)


def tail_diagnostics_dense(x: torch.Tensor, n_splits: int) -> dict:
    """x [C, S, m] -> the six outputs of ``tail_diagnostics`` in float64 (quantiles in x's dtype), all in torch."""
    ser = tail_series_dense(x)
    x64 = x.to(torch.float64)
    out = {'ess_bulk': multichain_ess_dense(ser['z'], n_splits), 'ess_mean': multichain_ess_dense(x64, n_splits)}
    lo, hi = multichain_ess_dense(ser['i_lo'].to(torch.float64), n_splits), multichain_ess_dense(ser['i_hi'].to(torch.float64), n_splits)
    out['ess_tail'] = torch.where(torch.isnan(lo) | torch.isnan(hi), torch.full_like(lo, float('nan')), torch.minimum(lo, hi))
    out['mcse_mean'] = x64.reshape(-1, x.shape[2]).std(dim=0, unbiased=True) / torch.sqrt(out['ess_mean'])
    out['rhat_folded'] = _split_r_hat_of_scores(ser['zf'], n_splits)
    out['quantiles'] = ser['quantiles']
    return out


def _tail_call(src: torch.Tensor, C: int, S: int, m: int, n_splits: int, what: int, **o):
    """mile_chain_diagnostics_tail on contiguous CUDA fp32 ``src`` ([C, S, m], or [m, C, S] with the plane bit in ``what``) with a
    workspace of the size it asks for; o: the output tensors, by name."""
    import ctypes as Ct
    from mile_amd import _lib
    lib = _lib.load_library()
    ptr = lambda t: Ct.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.device(src.device):
        ws = torch.empty(max(int(lib.mile_chain_diagnostics_tail_workspace(C, S, m, what)), 8), dtype=torch.uint8, device=src.device)
        stream = Ct.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
        _lib.check(lib.mile_chain_diagnostics_tail(ptr(src), C, S, m, n_splits, what, ptr(o.get('ess_bulk')), ptr(o.get('ess_tail')),
                                                   ptr(o.get('ess_mean')), ptr(o.get('mcse_mean')), ptr(o.get('rhat_folded')),
                                                   ptr(o.get('quantiles')), ptr(ws), ws.numel(), stream), lib)


def multichain_ess(series: torch.Tensor, n_splits: int = 2, plane: bool = False) -> torch.Tensor:
    """ESS_mc of given series, no ranking: series [C, S, m] (or [m, C, S] with ``plane``) -> [m].  CUDA fp32 runs in the
    library (mile_multichain_ess, at any C * S); anything else in ``multichain_ess_dense`` (float64)."""
    import ctypes as Ct
    from mile_amd import _lib
    m, C, S = (series.shape if plane else (series.shape[2], *series.shape[:2]))
    if not (series.is_cuda and series.dtype == torch.float32 and _lib.DIAG_S_MIN <= S <= _lib.DIAG_S_MAX):
        return multichain_ess_dense(series.permute(1, 2, 0) if plane else series, n_splits)
    lib = _lib.load_library()
    src = series.contiguous()
    ess = torch.empty(m, dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        ws = torch.empty(max(int(lib.mile_multichain_ess_workspace(C, S, m, int(plane))), 8), dtype=torch.uint8, device=src.device)
        stream = Ct.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)
        _lib.check(lib.mile_multichain_ess(Ct.c_void_p(src.data_ptr()), C, S, m, n_splits, int(plane), Ct.c_void_p(ess.data_ptr()),
                                           Ct.c_void_p(ws.data_ptr()), ws.numel(), stream), lib)
    return ess


def _tail_torch_sort(src: torch.Tensor, C: int, S: int, m: int, n_splits: int, plane: bool) -> dict:
    """The path past the library's pooled bound: per chunk of columns the series by torch sorts (``tail_series_dense`` on the
    fp32 draws), their ESS from mile_multichain_ess, R-hat of the folded scores from mile_chain_diagnostics' kernels."""
    from mile_amd._lib import DIAG_BITS as B
    new = lambda *sh: torch.empty(sh, dtype=torch.float32, device=src.device)
    out = {k: new(m) for k in TAIL_OUTPUTS}
    out['quantiles'] = new(3, m)
    step = max(1, (1 << 28) // (C * S * 8))                         # columns per sort: the int64 indices stay under 256 MB
    for k0 in range(0, m, step):
        xp = (src[k0:k0 + step].reshape(-1, C * S) if plane else src[:, :, k0:k0 + step].reshape(C * S, -1).t()).contiguous()
        k = xp.shape[0]
        ser = tail_series_plane(xp)                                  # rows [k, C * S]: the library's plane layout
        ess = multichain_ess(torch.cat([ser['z'].to(torch.float32), ser['i_lo'], ser['i_hi'], xp]).reshape(4 * k, C, S), n_splits,
                             plane=True)
        lo, hi = ess[k:2 * k], ess[2 * k:3 * k]
        sl = slice(k0, k0 + k)
        out['ess_bulk'][sl], out['ess_mean'][sl] = ess[:k], ess[3 * k:]
        out['ess_tail'][sl] = torch.where(torch.isnan(lo) | torch.isnan(hi), torch.full_like(lo, float('nan')), torch.minimum(lo, hi))
        sd = xp.to(torch.float64).std(dim=1, unbiased=True)
        out['mcse_mean'][sl] = (sd / torch.sqrt(ess[3 * k:].to(torch.float64))).to(torch.float32)
        r = new(k)
        _diag_call(ser['zf'].to(torch.float32).t().reshape(C, S, k).contiguous(), n_splits, B['rhat'] | B['pooled_input'], rhat=r)
        out['rhat_folded'][sl] = r
        out['quantiles'][:, sl] = ser['quantiles']
    return out


def tail_diagnostics(samples: torch.Tensor, n_splits: int = 2, plane: bool = False, torch_sort: bool = False) -> dict:
    """samples [C, S, ...] (with ``plane``: [m, C, S], the ``columns`` of ``function_diagnostics``) -> {'ess_bulk', 'ess_tail',
    'ess_mean', 'mcse_mean', 'rhat_folded' [...], 'quantiles' [3, ...] (q_lo, q_hi, median)}: the pooled multi-chain ESS of the
    rank-normalised draws, of the 5 % / 95 % tail indicators and of the draws, the Monte Carlo standard error of the mean, and the
    split R-hat of the draws folded about their median (include/mile_hip.h states each).  CUDA fp32 draws run in the library
    (mile_chain_diagnostics_tail; fp32 results), with torch sorts for the ranking past its pooled bound C * S > 16384 or when
    ``torch_sort`` asks for that path; anything else in torch (float64 results) -- CPU tensors, other dtypes, and, with a
    UserWarning, chains shorter than 4 or longer than 4096 draws."""
    global LAST_DTAIL_PATH
    import warnings
    from mile_amd._lib import DIAG_POOL_MAX, DIAG_S_MAX, DIAG_S_MIN, DTAIL_BITS
    if plane:
        m, C, S = samples.shape
        trail = (m,)
    else:
        C, S = samples.shape[:2]
        trail = tuple(samples.shape[2:])
    if S % n_splits:
        raise ValueError('Number of samples must be divisible by n_splits')
    if S // n_splits < 50:
        warnings.warn(message='Number of samples should be at least 50x the number of splits', category=UserWarning)
    in_range = DIAG_S_MIN <= S <= DIAG_S_MAX
    on_device = samples.is_cuda and samples.dtype == torch.float32
    if on_device and not in_range:
        warnings.warn(f'tail_diagnostics: {S} draws per chain is outside the range of the HIP kernels '
                      f'[{DIAG_S_MIN}, {DIAG_S_MAX}]; using the torch functions', category=UserWarning)
    if on_device and in_range:
        src = (samples if plane else samples.reshape(C, S, -1)).contiguous()
        m = src.shape[0] if plane else src.shape[2]
        if C * S <= DIAG_POOL_MAX and not torch_sort:
            out = {k: torch.empty(m, dtype=torch.float32, device=src.device) for k in TAIL_OUTPUTS}
            out['quantiles'] = torch.empty((3, m), dtype=torch.float32, device=src.device)
            what = sum(DTAIL_BITS[k] for k in ('ess_bulk', 'ess_tail', 'ess_mean', 'rhat_folded')) | (DTAIL_BITS['plane_input'] if plane else 0)
            _tail_call(src, C, S, m, n_splits, what, **out)
            LAST_DTAIL_PATH = 'library'
        else:
            out = _tail_torch_sort(src, C, S, m, n_splits, plane)
            LAST_DTAIL_PATH = 'library+torch_sort'
    else:
        x = (samples.permute(1, 2, 0) if plane else samples.reshape(C, S, -1)).contiguous()
        if not x.dtype.is_floating_point:
            x = x.to(torch.float64)
        out = tail_diagnostics_dense(x, n_splits)
        LAST_DTAIL_PATH = 'torch'
    return {k: v.reshape(*((3,) if k == 'quantiles' else ()), *trail) for k, v in out.items()}


def tail_diagnostics_summary(res: dict, n_draws: int, n_splits: int, rhat=None, prefix: str = 'dtail') -> dict:
    """The ``<prefix>_*`` scalars of a ``tail_diagnostics`` result over all its columns (non-finite cells skipped): min and median
    of ess_bulk and ess_tail, median and max of rhat_folded, the largest mcse_mean / sd (= 1 / sqrt(ess_mean)), the share
    median(ess_bulk) / n_draws, and, with ``rhat`` (the rank R-hat of ``chain_diagnostics`` on the same columns),
    ``rhat_rank_max``: the max over the columns of max(rhat, rhat_folded), the convergence figure of Vehtari et al."""
    import numpy as np
    a = {k: np.asarray(res[k].detach().cpu(), dtype=np.float64).reshape(-1) for k in TAIL_OUTPUTS}
    nan = float('nan')

    def stat(fn, v):
        v = v[np.isfinite(v)]
        return float(fn(v)) if v.size else nan
    out = {f'{prefix}_n_splits': int(n_splits)}
    for k in ('ess_bulk', 'ess_tail'):
        out[f'{prefix}_{k}_min'], out[f'{prefix}_{k}_median'] = stat(np.min, a[k]), stat(np.median, a[k])
    out[f'{prefix}_rhat_folded_median'], out[f'{prefix}_rhat_folded_max'] = stat(np.median, a['rhat_folded']), stat(np.max, a['rhat_folded'])
    if rhat is not None:
        r = np.asarray(rhat.detach().cpu() if hasattr(rhat, 'detach') else rhat, dtype=np.float64).reshape(-1)
        out[f'{prefix}_rhat_rank_max'] = stat(np.max, np.fmax(r, a['rhat_folded']))
    with np.errstate(all='ignore'):
        out[f'{prefix}_mcse_mean_over_sd_max'] = stat(np.max, 1.0 / np.sqrt(a['ess_mean']))
    out[f'{prefix}_ess_bulk_share'] = out[f'{prefix}_ess_bulk_median'] / float(n_draws)
    return out


# ---- canonical hidden-unit ordering of FCN draws: one representative of every draw's orbit under the permutations (and, for
# tanh, the sign flips) of its hidden units, so that the per-parameter statistics above mean something for chains that sit in
# permuted copies of one mode.  The rule is stated once, in include/mile_hip.h (mile_canonicalize_fcn); the library runs it on
# device tensors, the dense form here is the CPU statement, the timing yardstick and the path for very wide layers.

CANON_KEYS = ('bias', 'norm')
LAST_CANON_PATH = None      # how the last canonicalize call ran: 'library' or 'torch'


def _canon_check(spec, key: str, sign: bool):
    if not isinstance(spec, ModelSpec):
        raise ValueError(f'canonical ordering is defined for the FCN only, not for {type(spec).__name__}')
    if not spec.use_bias:
        raise ValueError('canonical ordering needs use_bias=True')
    if key not in CANON_KEYS:
        raise ValueError(f'key {key!r} (supported: {CANON_KEYS})')
    if sign and spec.activation != 'tanh':
        raise ValueError(f'sign fixing needs an odd activation: tanh only, not {spec.activation}')


def canonical_hidden(spec) -> int:
    """H: the hidden units of all hidden layers of the FCN ``spec`` (the last axis of ``perm`` and ``sign``)."""
    return int(sum(spec.hidden_structure[:-1]))


def canonicalize_dense(spec, theta: torch.Tensor, key: str = 'bias', sign: bool = False):
    """The rule of mile_canonicalize_fcn in torch, on whatever device ``theta`` [M, d] is on: a stable ``torch.sort`` of each
    hidden layer's keys (NaNs last), then ``take_along_dim`` of the bias, the columns and the next layer's rows.  Returns
    ``out`` [M, d] (theta's dtype), ``perm`` [M, H] int32, ``sign`` [M, H] int8."""
    _canon_check(spec, key, sign)
    M = theta.shape[0]
    leaves = {n.split('.', 1)[1]: (o, sh) for n, o, sh in spec.leaves()}
    nl = len(spec.hidden_structure)

    def layer(li):
        (ob, (fout,)), (ok, (fin, _)) = leaves[f'layer{li}.bias'], leaves[f'layer{li}.kernel']
        return ob, ok, fin, fout

    perms, signs = [], []
    for li in range(nl - 1):
        ob, ok, fin, fout = layer(li)
        b = theta[:, ob:ob + fout]
        s = torch.where(b < 0, -torch.ones_like(b), torch.ones_like(b)) if sign else torch.ones_like(b)
        if key == 'bias':
            k = s * b
        else:                                                   # fp64, the terms one after another: bias, then i ascending
            K = theta[:, ok:ok + fin * fout].reshape(M, fin, fout)
            k = b.double() * b.double()
            for i in range(fin):
                x = K[:, i, :].double()
                k = k + x * x
        p = torch.sort(k, dim=1, stable=True).indices
        perms.append(p)
        signs.append(torch.take_along_dim(s, p, dim=1))
    out = torch.empty_like(theta)
    for li in range(nl):
        ob, ok, fin, fout = layer(li)
        B = theta[:, ob:ob + fout]
        K = theta[:, ok:ok + fin * fout].reshape(M, fin, fout)
        if li < nl - 1:
            B = torch.take_along_dim(B, perms[li], dim=1) * signs[li]
            K = torch.take_along_dim(K, perms[li][:, None, :], dim=2) * signs[li][:, None, :]
        if li > 0:
            K = torch.take_along_dim(K, perms[li - 1][:, :, None], dim=1) * signs[li - 1][:, :, None]
        out[:, ob:ob + fout] = B
        out[:, ok:ok + fin * fout] = K.reshape(M, fin * fout)
    cat = lambda ts, dt: (torch.cat(ts, dim=1) if ts else torch.empty((M, 0), device=theta.device)).to(dt)
    return out, cat(perms, torch.int32), cat(signs, torch.int8)


def _library_canonicalize(spec, theta: torch.Tensor, key: str, sign: bool, want_index: bool):
    """theta [M, d] contiguous CUDA fp32 -> (out, perm, sign) from mile_canonicalize_fcn (perm, sign None unless wanted)."""
    import ctypes as Ct
    from mile_amd import _lib
    lib = _lib.load_library()
    cs = _lib.fcn_spec_c(spec)
    M, H = theta.shape[0], canonical_hidden(spec)
    how = _lib.CANON_BITS[key] | (_lib.CANON_BITS['sign'] if sign else 0)
    ptr = lambda t: Ct.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.device(theta.device):
        out = torch.empty_like(theta)
        perm = torch.empty((M, H), dtype=torch.int32, device=theta.device) if want_index else None
        sgn = torch.empty((M, H), dtype=torch.int8, device=theta.device) if want_index else None
        nws = int(lib.mile_canonicalize_fcn_workspace(Ct.byref(cs), M, how))
        if nws < 0:
            _lib.check(-1, lib)
        ws = torch.empty(nws, dtype=torch.uint8, device=theta.device) if nws else None
        stream = Ct.c_void_p(torch.cuda.current_stream(theta.device).cuda_stream)
        _lib.check(lib.mile_canonicalize_fcn(Ct.byref(cs), ptr(theta), M, how, ptr(out), ptr(perm), ptr(sgn), ptr(ws), nws, stream), lib)
    return out, perm, sgn


def canonicalize(spec, theta: torch.Tensor, key: str = 'bias', sign: bool = False, return_perm: bool = False):
    """theta [C, S, d] or [M, d] draws of the FCN ``spec`` -> the canonical draws in the same shape: hidden units of every
    layer in ascending order of ``key`` ('bias': the unit's bias; 'norm': the squared norm of its bias and incoming weights),
    with ``sign`` (tanh only) every unit's bias made non-negative first.  With ``return_perm`` also ``perm`` [..., H] int32 (the
    original index of the unit at each position) and ``sign`` [..., H] int8.  CUDA fp32 draws run in the library
    (mile_canonicalize_fcn), anything else -- and, with a UserWarning, nets with a hidden layer wider than 1024 -- in
    ``canonicalize_dense``.  Ordering by a key gives order statistics, not an alignment to a reference mode: where two units'
    keys cross inside a chain the labels switch (see ``permutation_switches``)."""
    global LAST_CANON_PATH
    import warnings
    from mile_amd._lib import CANON_WIDTH_MAX
    _canon_check(spec, key, sign)
    if theta.dim() not in (2, 3) or theta.shape[-1] != spec.n_params:
        raise ValueError(f'theta must be [C, S, {spec.n_params}] or [M, {spec.n_params}], got {tuple(theta.shape)}')
    flat = theta.reshape(-1, theta.shape[-1])
    wide = max(spec.hidden_structure[:-1], default=0) > CANON_WIDTH_MAX
    on_device = theta.is_cuda and theta.dtype == torch.float32
    if on_device and wide:
        warnings.warn(f'canonicalize: a hidden layer wider than {CANON_WIDTH_MAX} is outside the range of the HIP kernels; '
                      'using the torch form', category=UserWarning)
    if on_device and not wide:
        out, perm, sgn = _library_canonicalize(spec, flat.contiguous(), key, sign, return_perm)
        LAST_CANON_PATH = 'library'
    else:
        out, perm, sgn = canonicalize_dense(spec, flat, key, sign)
        LAST_CANON_PATH = 'torch'
    out = out.reshape(theta.shape)
    if not return_perm:
        return out
    lead = tuple(theta.shape[:-1])
    return out, perm.reshape(*lead, -1), sgn.reshape(*lead, -1)


def permutation_switches(perm: torch.Tensor, spec) -> torch.Tensor:
    """perm [C, S, H] -> int64 [C, n_hidden]: for each chain and hidden layer the draws j >= 1 whose order differs from that of
    draw j - 1.  The label-switching count: near 0 the key separates the units of this posterior and the canonical parameters
    are the same units throughout; a large share means the per-parameter statistics are those of order statistics."""
    perm = torch.as_tensor(perm)
    widths = list(spec.hidden_structure[:-1])
    if perm.dim() != 3 or perm.shape[2] != sum(widths):
        raise ValueError(f'perm must be [C, S, {sum(widths)}], got {tuple(perm.shape)}')
    out = torch.zeros((perm.shape[0], len(widths)), dtype=torch.int64, device=perm.device)
    o = 0
    for l, w in enumerate(widths):
        span = perm[:, :, o:o + w]
        out[:, l] = (span[:, 1:] != span[:, :-1]).any(dim=2).sum(dim=1)
        o += w
    return out


def canonical_diagnostics(spec, samples: torch.Tensor, n_splits: int = 2, key: str = 'bias', sign: bool = False) -> dict:
    """samples [C, S, d] -> ``chain_diagnostics`` of the canonical draws (``canonicalize``), plus 'switches' [C, n_hidden]
    (``permutation_switches``)."""
    out, perm, _ = canonicalize(spec, samples, key, sign, return_perm=True)
    res = chain_diagnostics(out, n_splits)
    res['switches'] = permutation_switches(perm, spec)
    return res


# ---- alignment to a reference draw by hidden-unit assignment: the other half of the above.  Every draw's hidden units are
# matched to those of ONE reference row by a linear assignment problem per layer, so that "parameter j" is the same unit in
# every draw and chain.  The rule is stated once, in include/mile_hip.h (mile_align_fcn); the library runs it on device tensors
# (hidden widths up to 128), the dense form here is the yardstick and the path for everything else.

LAST_ALIGN_PATH = None      # how the last align call ran: 'library' or 'scipy'


def _align_check(spec, sign: bool):
    if not isinstance(spec, ModelSpec):
        raise ValueError(f'alignment to a reference draw is defined for the FCN only, not for {type(spec).__name__}')
    if not spec.use_bias:
        raise ValueError('alignment to a reference draw needs use_bias=True')
    if sign and spec.activation != 'tanh':
        raise ValueError(f'sign fixing needs an odd activation: tanh only, not {spec.activation}')


def align_dense(spec, theta: torch.Tensor, reference: torch.Tensor, sign: bool = False):
    """The rule of mile_align_fcn with torch and scipy, on whatever device ``theta`` [M, d] is on: per hidden layer the
    similarities of all draws as one fp64 matrix product, then ``scipy.optimize.linear_sum_assignment`` per draw on the host, then
    ``take_along_dim`` of the bias, the columns and the next layer's rows.  Returns ``out`` [M, d] (theta's dtype), ``perm``
    [M, H] int32, ``sign`` [M, H] int8, ``score`` [M, n_hidden] fp64, ``dropped`` [M] int32.

    The matrix product adds the terms of a similarity in its own order and scipy breaks ties between equally good assignments in
    its own way, so this form need not give the library's permutation where two assignments tie (or nearly tie); each layer's
    objective is the same maximum."""
    import numpy as np
    from scipy.optimize import linear_sum_assignment
    _align_check(spec, sign)
    M, dev = theta.shape[0], theta.device
    ref = torch.as_tensor(reference).to(dev).reshape(-1)
    if ref.shape[0] != spec.n_params:
        raise ValueError(f'reference must hold {spec.n_params} floats, got {tuple(ref.shape)}')
    leaves = {n.split('.', 1)[1]: (o, sh) for n, o, sh in spec.leaves()}
    nl = len(spec.hidden_structure)
    nh = nl - 1

    def layer(li):
        (ob, (fout,)), (ok, (fin, _)) = leaves[f'layer{li}.bias'], leaves[f'layer{li}.kernel']
        return ob, ok, fin, fout

    t64, r64 = theta.double(), ref.double()
    ok_rows = torch.ones(M, dtype=torch.bool, device=dev)
    perms, signs, scores = [], [], []
    for li in range(nh):
        ob, ok, fin, W = layer(li)
        Kd = t64[:, ok:ok + fin * W].reshape(M, fin, W)
        if li > 0:
            Kd = torch.take_along_dim(Kd, perms[-1][:, :, None], dim=1) * signs[-1][:, :, None]
        Fr = torch.cat([r64[ob:ob + W][None], r64[ok:ok + fin * W].reshape(fin, W)], dim=0)                # [1 + fin, W]
        Fd = torch.cat([t64[:, None, ob:ob + W], Kd], dim=1)                                              # [M, 1 + fin, W]
        if li == nh - 1:
            _, ok2, fin2, O = layer(li + 1)
            Fr = torch.cat([Fr, r64[ok2:ok2 + fin2 * O].reshape(fin2, O).T], dim=0)
            Fd = torch.cat([Fd, t64[:, ok2:ok2 + fin2 * O].reshape(M, fin2, O).transpose(1, 2)], dim=1)
        p = torch.arange(W, device=dev).repeat(M, 1)
        hit = torch.empty((M, W), dtype=torch.float64, device=dev)
        step = max(1, (1 << 27) // (W * W))                                                                # 1 GiB of fp64 at a time
        for m0 in range(0, M, step):
            S = torch.matmul(Fr.T[None], Fd[m0:m0 + step])                                                 # [m, W, W]
            fin_rows = torch.isfinite(S).all(dim=2).all(dim=1)
            ok_rows[m0:m0 + step] &= fin_rows
            G = (S.abs() if sign else S).cpu().numpy()
            alive = ok_rows[m0:m0 + step].cpu().numpy()
            pc = np.tile(np.arange(W), (G.shape[0], 1))
            for m in range(G.shape[0]):
                if alive[m]:
                    pc[m] = linear_sum_assignment(G[m], maximize=True)[1]
            p[m0:m0 + step] = torch.from_numpy(pc).to(dev)
            hit[m0:m0 + step] = torch.take_along_dim(S, p[m0:m0 + step, :, None], dim=2)[:, :, 0]
        s = torch.where(hit < 0, -torch.ones_like(hit), torch.ones_like(hit)) if sign else torch.ones_like(hit)
        perms.append(p), signs.append(s), scores.append((hit.abs() if sign else hit).sum(dim=1))
    out = torch.empty_like(theta)
    for li in range(nl):
        ob, ok, fin, fout = layer(li)
        B = theta[:, ob:ob + fout]
        K = theta[:, ok:ok + fin * fout].reshape(M, fin, fout)
        if li < nh:
            sg = signs[li].to(theta.dtype)
            B = torch.take_along_dim(B, perms[li], dim=1) * sg
            K = torch.take_along_dim(K, perms[li][:, None, :], dim=2) * sg[:, None, :]
        if li > 0:
            K = torch.take_along_dim(K, perms[li - 1][:, :, None], dim=1) * signs[li - 1].to(theta.dtype)[:, :, None]
        out[:, ob:ob + fout] = B
        out[:, ok:ok + fin * fout] = K.reshape(M, fin * fout)
    cat = lambda ts, dt: (torch.cat(ts, dim=1) if ts else torch.empty((M, 0), device=dev)).to(dt)
    perm, sgn = cat(perms, torch.int32), cat(signs, torch.int8)
    score = torch.stack(scores, dim=1) if scores else torch.empty((M, 0), dtype=torch.float64, device=dev)
    # a draw with a non-finite similarity in any layer is copied: identity, +1, NaN scores
    bad = ~ok_rows
    if bool(bad.any()):
        ident = torch.cat([torch.arange(w, device=dev) for w in spec.hidden_structure[:-1]]).to(torch.int32)
        out[bad], perm[bad], sgn[bad], score[bad] = theta[bad], ident, 1, float('nan')
    return out, perm, sgn, score, bad.to(torch.int32)


def _library_align(spec, theta: torch.Tensor, reference: torch.Tensor, sign: bool, want_index: bool = True, want_score: bool = True):
    """theta [M, d], reference [d] contiguous CUDA fp32 -> (out, perm, sign, score, dropped) from mile_align_fcn (perm and sign,
    and score, None unless wanted)."""
    import ctypes as Ct
    from mile_amd import _lib
    lib = _lib.load_library()
    cs = _lib.fcn_spec_c(spec)
    M, H, nh = theta.shape[0], canonical_hidden(spec), len(spec.hidden_structure) - 1
    how = _lib.ALIGN_SIGN if sign else 0
    ptr = lambda t: Ct.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.device(theta.device):
        out = torch.empty((M, theta.shape[1]), dtype=torch.float32, device=theta.device)
        perm = torch.empty((M, H), dtype=torch.int32, device=theta.device) if want_index else None
        sgn = torch.empty((M, H), dtype=torch.int8, device=theta.device) if want_index else None
        score = torch.empty((M, nh), dtype=torch.float64, device=theta.device) if want_score else None
        dropped = torch.empty(M, dtype=torch.int32, device=theta.device)
        nws = int(lib.mile_align_fcn_workspace(Ct.byref(cs), M, how))
        if nws < 0:
            _lib.check(-1, lib)
        ws = torch.empty(nws, dtype=torch.uint8, device=theta.device) if nws else None
        stream = Ct.c_void_p(torch.cuda.current_stream(theta.device).cuda_stream)
        _lib.check(lib.mile_align_fcn(Ct.byref(cs), ptr(theta), M, ptr(reference), how, ptr(out), ptr(perm), ptr(sgn), ptr(score),
                                      ptr(dropped), ptr(ws), nws, stream), lib)
    return out, perm, sgn, score, dropped


def align(spec, theta: torch.Tensor, reference='first', rounds: int = 1, sign: bool = False) -> dict:
    """theta [C, S, d] or [M, d] draws of the FCN ``spec`` -> every draw with its hidden units matched to those of ``reference``
    ('first': the first draw; or a tensor of d floats) by one linear assignment problem per hidden layer, solved in a forward
    sweep; with ``sign`` (tanh only) a matched unit that points the other way is flipped.  ``rounds`` >= 2 repeats the alignment
    of the ORIGINAL draws, round r to the fp64 mean of round r - 1's aligned draws (those not dropped) cast to fp32.  Returns a
    dict: 'theta' (theta's shape), 'perm' [..., H] int32 (the draw's unit at each reference position), 'sign' [..., H] int8,
    'score' [..., n_hidden] fp64 (the matched similarity per layer), 'dropped' [...] int32 (draws with a non-finite similarity:
    copied unchanged, NaN scores) and 'reference' [d], the row the last round aligned to.  CUDA fp32 draws of nets whose hidden
    widths are at most 128 run in the library (mile_align_fcn); anything else -- wider nets with a UserWarning -- in
    ``align_dense``, which may break ties differently."""
    global LAST_ALIGN_PATH
    import warnings
    from mile_amd._lib import ALIGN_WIDTH_MAX
    _align_check(spec, sign)
    if theta.dim() not in (2, 3) or theta.shape[-1] != spec.n_params:
        raise ValueError(f'theta must be [C, S, {spec.n_params}] or [M, {spec.n_params}], got {tuple(theta.shape)}')
    if int(rounds) < 1:
        raise ValueError(f'rounds must be at least 1, got {rounds}')
    flat = theta.reshape(-1, theta.shape[-1])
    if isinstance(reference, str):
        if reference != 'first':
            raise ValueError(f"reference {reference!r} (supported: 'first' or a tensor of {spec.n_params} floats)")
        ref = flat[0].clone()
    else:
        ref = torch.as_tensor(reference).to(flat.device, flat.dtype).reshape(-1).clone()
        if ref.shape[0] != spec.n_params:
            raise ValueError(f'reference must hold {spec.n_params} floats, got {tuple(ref.shape)}')
    wide = max(spec.hidden_structure[:-1], default=0) > ALIGN_WIDTH_MAX
    on_device = theta.is_cuda and theta.dtype == torch.float32
    if on_device and wide:
        warnings.warn(f'align: a hidden layer wider than {ALIGN_WIDTH_MAX} is outside the range of the HIP kernel; using scipy on '
                      'the host', category=UserWarning)
    for r in range(int(rounds)):
        if on_device and not wide:
            res = _library_align(spec, flat.contiguous(), ref.contiguous(), sign)
            LAST_ALIGN_PATH = 'library'
        else:
            res = align_dense(spec, flat, ref, sign)
            LAST_ALIGN_PATH = 'scipy'
        used = ref
        keep = res[4] == 0
        if r + 1 < int(rounds) and bool(keep.any()):
            ref = res[0][keep].double().mean(dim=0).to(flat.dtype)
    lead = tuple(theta.shape[:-1])
    out, perm, sgn, score, dropped = res
    return {'theta': out.reshape(theta.shape), 'perm': perm.reshape(*lead, -1), 'sign': sgn.reshape(*lead, -1),
            'score': score.reshape(*lead, -1), 'dropped': dropped.reshape(lead), 'reference': used}


def aligned_diagnostics(spec, samples: torch.Tensor, n_splits: int = 2, reference='first', rounds: int = 2, sign: bool = False) -> dict:
    """samples [C, S, d] -> ``chain_diagnostics`` of the draws aligned to ``reference`` (``align``), plus 'switches' [C, n_hidden]
    (``permutation_switches`` of the returned perms: 0 where a chain keeps one matching throughout), 'score_mean' [n_hidden] (the
    mean matched similarity per layer over the draws kept), 'scores' [C, S, n_hidden], 'dropped' (a count), 'reference' [d] and
    'theta', the aligned draws."""
    if samples.dim() != 3:
        raise ValueError(f'samples must be [C, S, d], got {tuple(samples.shape)}')
    al = align(spec, samples, reference, rounds, sign)
    res = chain_diagnostics(al['theta'], n_splits)
    res['switches'] = permutation_switches(al['perm'], spec)
    res['score_mean'] = torch.nanmean(al['score'].reshape(-1, al['score'].shape[-1]), dim=0)
    res['scores'], res['reference'], res['theta'] = al['score'], al['reference'], al['theta']
    res['dropped'] = int(al['dropped'].sum())
    return res


# ---- chain diagnostics in function space: the statistics above, of what every draw predicts on every row.  The library
# streams them (Engine.function_diagnostics, mile_function_diagnostics); the dense forms here are the yardstick and the path
# for CPU tensors.

def function_columns_dense(outputs: torch.Tensor, y, task: str) -> torch.Tensor:
    """outputs [C, S, N, O] (``predict``'s tensor) -> the series [C, S, M] in outputs' dtype.  With Q = O + 1 (Q = O when ``y``
    is None) column n * Q + q is quantity q of row n: regression (mu, log sigma, l), classification (the O softmax
    probabilities exp(z_k - (m + log(se))), l), l = log p(y_n | x_n, theta) with sigma clipped to [1e-6, 1e6] as in
    ``pointwise_loglik``.  With ``y`` the last column is L = sum_n l_n, summed in float64 in row order."""
    z = outputs
    C_, S_, N, O = z.shape
    if task == 'regr':
        parts = [z]
        if y is not None:
            yt = torch.as_tensor(y, device=z.device).to(z.dtype).reshape(N)
            es = torch.exp(z[..., 1])
            sig = torch.where(torch.isnan(es), es, es.clamp(1e-6, 1e6))
            r = (yt - z[..., 0]) / sig
            ll = -0.5 * r * r - torch.log(sig) - 0.91893853320467274
    else:
        m = z.max(dim=-1, keepdim=True).values
        lse = m + torch.log(torch.exp(z - m).sum(dim=-1, keepdim=True))
        parts = [torch.exp(z - lse)]
        if y is not None:
            yi = torch.as_tensor(y, device=z.device).to(torch.int64).reshape(1, 1, N, 1).expand(C_, S_, N, 1)
            ll = (torch.gather(z, 3, yi) - lse)[..., 0]
    if y is None:
        return parts[0].reshape(C_, S_, N * O)
    cols = torch.cat([parts[0], ll[..., None]], dim=-1).reshape(C_, S_, N * (O + 1))
    L = torch.cumsum(ll.to(torch.float64), dim=-1)[..., -1:]              # row after row, as the library adds them
    return torch.cat([cols, L.to(z.dtype)], dim=-1)


def _function_summaries(rhat, crhat, ess, NQ: int):
    """(summary dict keyed by _lib.FDIAG_SUMMARY, chain_summary [C, 2] float64) of statistic arrays rhat [M], crhat, ess [C, M]
    over their first NQ columns: what k_fdiag_summary reduces on the device, for the paths that do not run it.  Non-finite
    cells are skipped and counted; of equal extremes the lower chain, then the lower column wins."""
    import numpy as np
    r = rhat.detach().cpu().numpy().astype(np.float64)[:NQ]
    c = crhat.detach().cpu().numpy().astype(np.float64)[:, :NQ]
    e = ess.detach().cpu().numpy().astype(np.float64)[:, :NQ]
    nan = float('nan')

    def extreme(a, fin, largest):
        if not fin.any():
            return nan, -1
        b = np.where(fin, a, -np.inf if largest else np.inf).reshape(-1)
        i = int(np.argmax(b) if largest else np.argmin(b))               # the first of equal extremes in C order
        return float(b[i]), i
    fr, fc, fe = np.isfinite(r), np.isfinite(c), np.isfinite(e)
    rmax, ri = extreme(r, fr, True)
    cmax, ci = extreme(c, fc, True)
    emin, ei = extreme(e, fe, False)
    s = {'rhat_max': rmax, 'rhat_mean': float(r[fr].sum() / fr.sum()) if fr.any() else nan, 'rhat_column': float(ri),
         'rhat_gt_1_01': float((r[fr] > 1.01).sum()), 'rhat_gt_1_05': float((r[fr] > 1.05).sum()),
         'rhat_gt_1_1': float((r[fr] > 1.1).sum()), 'rhat_skipped': float((~fr).sum()),
         'crhat_max': cmax, 'crhat_chain': float(ci // NQ if ci >= 0 else -1), 'crhat_column': float(ci % NQ if ci >= 0 else -1),
         'crhat_skipped': float((~fc).sum()),
         'ess_min': emin, 'ess_mean': float(e[fe].sum() / fe.sum()) if fe.any() else nan,
         'ess_chain': float(ei // NQ if ei >= 0 else -1), 'ess_column': float(ei % NQ if ei >= 0 else -1),
         'ess_skipped': float((~fe).sum())}
    chain = np.stack([np.where(fe.any(axis=1), np.where(fe, e, np.inf).min(axis=1), nan),
                      np.where(fc.any(axis=1), np.where(fc, c, -np.inf).max(axis=1), nan)], axis=1)
    return s, torch.from_numpy(chain)


def function_diagnostics_dense(outputs: torch.Tensor, y, task: str, n_splits: int = 2) -> dict:
    """``chain_diagnostics`` of ``function_columns_dense(outputs, y, task)``, as the dict ``Engine.function_diagnostics``
    returns (``columns`` [M, C, S] always there): the composition that holds every tensor at once, which the library call is
    measured against, and the path for CPU tensors (float64 statistics then)."""
    cols = function_columns_dense(outputs, y, task)
    C_, S_, N, O = outputs.shape
    Q = O + (1 if y is not None else 0)
    res = dict(chain_diagnostics(cols, n_splits))
    res['columns'] = cols.permute(2, 0, 1).contiguous()
    res['loglik_sum'] = None
    if y is not None:
        ll = cols[:, :, :N * Q].reshape(C_, S_, N, Q)[..., O]
        res['loglik_sum'] = torch.cumsum(ll.to(torch.float64), dim=-1)[..., -1]
    res['summary'], res['chain_summary'] = _function_summaries(res['rhat'], res['crhat'], res['ess'], N * Q)
    res['Q'], res['M'] = Q, int(cols.shape[2])
    return res


LAST_FDIAG_PATH = None      # how the last function_diagnostics call ran: 'library' or 'library+torch_sort'


def function_diagnostics(eng, samples, x, y=None, n_splits: int = 2, return_columns: bool = False, max_draws_per_pass: int = 0,
                         max_rows_per_tile: int = 0, block_rows: int = 0) -> dict:
    """All five statistics of ``Engine.function_diagnostics`` for samples [C, S, d] at any C * S.  Up to the library's pooled
    bound (C * S <= 16384) this is one library call.  Past it the rows go in blocks of ``block_rows`` (0: as many as keep a
    block's columns under 256 MB): the library gives wcv, bcv, crhat, the columns and the block's summed log-likelihood, the
    columns are ranked by the torch sort that ``chain_diagnostics`` uses there and go back into the library's ESS / R-hat
    kernels; the blocks' log-likelihood sums are added in block order, and that column gets its statistics last.  Inside a
    block the library adds the rows in row order; across blocks the fp64 sums associate by block, so ``loglik_sum`` (and the
    last column's statistics) equal the one-call, row-order sum bit for bit only while every block after the first holds one
    row, and to fp64 rounding otherwise: unlike the library's tiles, ``block_rows`` can move the last bits of that column."""
    global LAST_FDIAG_PATH
    from mile_amd._lib import DIAG_POOL_MAX
    samples = torch.as_tensor(samples)
    C_, S_ = int(samples.shape[0]), int(samples.shape[1])
    caps = dict(max_draws_per_pass=max_draws_per_pass, max_rows_per_tile=max_rows_per_tile)
    if C_ * S_ <= DIAG_POOL_MAX:
        LAST_FDIAG_PATH = 'library'
        return eng.function_diagnostics(samples, x, y, n_splits=n_splits, return_columns=return_columns, **caps)
    x = torch.as_tensor(x)
    N = int(x.shape[0])
    O = int(eng.spec.hidden_structure[-1])
    Q = O + (1 if y is not None else 0)
    M = N * Q + (1 if y is not None else 0)
    nb = int(block_rows) if block_rows else max(1, (1 << 28) // (C_ * S_ * 4 * Q))
    dev = eng.device
    samples = samples.to(dev)
    y = None if y is None else torch.as_tensor(y)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    out = {'wcv': new(M), 'bcv': new(M), 'rhat': new(M), 'ess': new(C_, M), 'crhat': new(C_, M),
           'columns': new(M, C_, S_) if return_columns else None, 'loglik_sum': None}
    total = torch.zeros((C_, S_), dtype=torch.float64, device=dev) if y is not None else None
    for r0 in range(0, N, nb):
        r1 = min(N, r0 + nb)
        blk = eng.function_diagnostics(samples, x[r0:r1], None if y is None else y[r0:r1], n_splits=n_splits,
                                       what=('wcv', 'bcv', 'crhat'), return_columns=True, **caps)
        m0, m1 = r0 * Q, r1 * Q                                          # (the block's own last column, its L, is left out)
        for k in ('wcv', 'bcv'):
            out[k][m0:m1] = blk[k][:m1 - m0]
        out['crhat'][:, m0:m1] = blk['crhat'][:, :m1 - m0]
        cols = blk['columns'][:m1 - m0]
        out['ess'][:, m0:m1], out['rhat'][m0:m1] = _pooled_ess_rhat(cols.permute(1, 2, 0).contiguous(), n_splits)
        if return_columns:
            out['columns'][m0:m1] = cols
        if y is not None:
            total += blk['loglik_sum']
    if y is not None:
        L = total.to(torch.float32)[:, :, None].contiguous()
        last = _library_diagnostics(L, n_splits)
        for k in ('wcv', 'bcv', 'rhat'):
            out[k][M - 1] = last[k][0]
        for k in ('ess', 'crhat'):
            out[k][:, M - 1] = last[k][:, 0]
        if return_columns:
            out['columns'][M - 1] = L[:, :, 0]
        out['loglik_sum'] = total
    out['summary'], cs = _function_summaries(out['rhat'], out['crhat'], out['ess'], N * Q)
    out['chain_summary'] = cs.to(dev)
    out['Q'], out['M'] = Q, M
    LAST_FDIAG_PATH = 'library+torch_sort'
    return out


def function_quantity_names(task: str, O: int, with_y: bool) -> list:
    """The names of the Q quantities of a row, in column order."""
    names = ['mu', 'log_sigma'] if task == 'regr' else [f'p{k}' for k in range(O)]
    return names + (['loglik'] if with_y else [])


def function_diagnostics_summary(res: dict, N: int, Q: int, task: str = 'regr') -> dict:
    """The ``fdiag_*`` scalars of a ``function_diagnostics`` result on N rows with Q quantities each: the library's summary
    (max / mean R-hat and its column, the columns above 1.01 / 1.05 / 1.1, max per-chain R-hat, min / mean ESS, the cells
    skipped), per quantity the max / mean R-hat and min ESS, the summed log-likelihood's own R-hat and ESS, the mean share of
    the between-chain variance bcv / (bcv + wcv), and ``fdiag_r_eff_mean``: the mean over the rows of sum_c ess[c, l_n] /
    (C * S), the relative efficiency PSIS-LOO asks for when the rows are the training rows."""
    import numpy as np
    arr = {k: res[k].detach().cpu().numpy().astype(np.float64) for k in ('wcv', 'bcv', 'rhat', 'ess', 'crhat')}
    NQ, M = N * Q, int(res['M'])
    with_y = M > NQ
    C_ = arr['ess'].shape[0]
    out = {f'fdiag_{k}': (int(v) if k.endswith(('_column', '_chain', '_skipped')) or '_gt_' in k else float(v))
           for k, v in res['summary'].items()}
    out['fdiag_n_columns'] = M
    with np.errstate(all='ignore'):
        for q, name in enumerate(function_quantity_names(task, Q - (1 if with_y else 0), with_y)):
            r, e = arr['rhat'][q:NQ:Q], arr['ess'][:, q:NQ:Q]
            out[f'fdiag_rhat_max_{name}'] = float(np.nanmax(r)) if np.isfinite(r).any() else float('nan')
            out[f'fdiag_rhat_mean_{name}'] = float(np.nanmean(r)) if np.isfinite(r).any() else float('nan')
            out[f'fdiag_ess_min_{name}'] = float(np.nanmin(e)) if np.isfinite(e).any() else float('nan')
        share = arr['bcv'][:NQ] / (arr['bcv'][:NQ] + arr['wcv'][:NQ])
        out['fdiag_between_share'] = float(np.nanmean(share)) if np.isfinite(share).any() else float('nan')
    if with_y:
        out['fdiag_loglik_sum_rhat'] = float(arr['rhat'][M - 1])
        out['fdiag_loglik_sum_ess'] = float(arr['ess'][:, M - 1].sum())
        if res.get('loglik_sum') is not None:
            S_ = int(res['loglik_sum'].shape[1])
            out['fdiag_r_eff_mean'] = float(np.mean(arr['ess'][:, Q - 1:NQ:Q].sum(axis=0) / (C_ * S_)))
    out['fdiag_chain_ess_min'] = [float(v) for v in res['chain_summary'][:, 0].cpu()]
    out['fdiag_chain_crhat_max'] = [float(v) for v in res['chain_summary'][:, 1].cpu()]
    return out


# ---- the rest of evaluate_bde's report (src/inference/evaluation.py:46-137,409-544): draws from the raw outputs of
# Engine.predict, then ACC, RMSE, coverage and calibration error.  Plain torch on the tensors' device, no loop over samples.

def sample_from_predictions(preds: torch.Tensor, task: str, generator: torch.Generator | None = None) -> torch.Tensor:
    """preds [..., N, O] raw outputs -> one posterior-predictive draw per (sample, row) [..., N] (evaluation.py:46-71).
    Regression: ``z * clip(exp(log sigma), 1e-6, 1e6) + mu`` with ``z = torch.randn(mu.shape, generator=generator)``.
    Classification: a categorical draw from the logits by the Gumbel-max rule (what jax.random.categorical does), int64.
    The draws come from the torch generator handed in (on the tensors' device): the reference's jax.random key 42 cannot be
    reproduced here, as for the sampler's noise, so metrics built on the draws agree in distribution, not draw by draw."""
    if task in ('regr', 'regression'):
        loc = preds[..., 0]
        scale = torch.exp(preds[..., 1]).clamp(min=1e-6, max=1e6)
        z = torch.randn(loc.shape, generator=generator, dtype=loc.dtype, device=loc.device)
        return z * scale + loc
    e = torch.empty_like(preds).exponential_(generator=generator)       # -log(e) is a standard Gumbel variate
    return torch.argmax(preds - torch.log(e), dim=-1)


def class_counts(draws: torch.Tensor, n_classes: int) -> torch.Tensor:
    """draws [..., N] integer labels -> [N, n_classes] int64: how often each class was drawn for each row, over all leading
    axes.  Counts of disjoint sets of samples add, so a caller may accumulate them over chunks of samples."""
    N = draws.shape[-1]
    flat = draws.reshape(-1, N).to(torch.int64)
    key = flat + torch.arange(N, device=flat.device, dtype=torch.int64) * n_classes
    return torch.bincount(key.reshape(-1), minlength=N * n_classes).reshape(N, n_classes)


def accuracy_from_counts(counts: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """counts [..., N, K] -> mean(labels == most drawn class) over the rows, [...].  Ties go to the SMALLEST label, as
    scipy.stats.mode does: the count and the label are packed into one key whose maximum is unique."""
    K = counts.shape[-1]
    key = counts.to(torch.int64) * K + (K - 1 - torch.arange(K, device=counts.device, dtype=torch.int64))
    mode = torch.argmax(key, dim=-1)
    return (mode == labels.to(counts.device, torch.int64)).to(torch.float64).mean(dim=-1)


def accuracy(draws: torch.Tensor, labels: torch.Tensor, n_classes: int | None = None) -> torch.Tensor:
    """mean(labels == mode of the drawn labels over all leading axes) (evaluation.py:470-472,487), draws [..., N]."""
    if n_classes is None:
        n_classes = int(max(int(draws.max()), int(labels.max()))) + 1
    return accuracy_from_counts(class_counts(draws, n_classes), labels)


def get_quantiles(coverage: float) -> torch.Tensor:
    """The two quantile levels of the central interval of a nominal coverage (evaluation.py:96-98)."""
    return torch.tensor([0.5 - coverage / 2, 0.5 + coverage / 2], dtype=torch.float64)


def coverage_weighting(nominal_coverage, kappa: float = 1.0) -> torch.Tensor:
    """nominal ** kappa, normalised to sum 1 (evaluation.py:87-93)."""
    nc = torch.as_tensor(nominal_coverage, dtype=torch.float64)
    return nc ** kappa / torch.sum(nc ** kappa)


def _quantiles_linear(flat: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """flat [M, N], q [Q] in [0, 1] -> [Q, N]: linear interpolation between order statistics (numpy's default method, same
    arithmetic).  A sort, not torch.quantile, whose input size is capped."""
    M = flat.shape[0]
    sv = torch.sort(flat, dim=0).values
    pos = q.to(torch.float64) * (M - 1)
    lo = torch.floor(pos)
    t = (pos - lo).to(flat.dtype)[:, None].to(flat.device)
    lo = lo.to(torch.int64).to(flat.device)
    hi = torch.clamp(lo + 1, max=M - 1)
    a, b = sv[lo], sv[hi]
    d = b - a
    return torch.where(t >= 0.5, b - d * (1 - t), a + d * t)


def calculate_coverage(nominal_coverages, y: torch.Tensor, draws: torch.Tensor) -> torch.Tensor:
    """Observed coverage of the central credible intervals (evaluation.py:101-137): draws [..., N] (all leading axes are
    pooled: C * S draws per row), y [N] -> [len(nominal_coverages)] float64.  Both interval bounds are inclusive."""
    flat = draws.reshape(-1, draws.shape[-1])
    y = y.to(flat.device, flat.dtype)
    q = torch.stack([get_quantiles(float(c)) for c in nominal_coverages])          # [n, 2]
    creds = _quantiles_linear(flat, q.reshape(-1)).reshape(len(nominal_coverages), 2, -1)
    inside = (creds[:, 0] <= y) & (creds[:, 1] >= y)
    return inside.to(torch.float64).mean(dim=1)


def calibration_error(nominal_coverage, observed_coverage, weights=None) -> torch.Tensor:
    """sqrt(mean(w * (nominal - observed)^2)), w = 1 without weights (evaluation.py:74-84)."""
    obs = torch.as_tensor(observed_coverage, dtype=torch.float64)
    sq = (torch.as_tensor(nominal_coverage, dtype=torch.float64).to(obs.device) - obs) ** 2
    if weights is not None:
        sq = torch.as_tensor(weights, dtype=torch.float64).to(obs.device) * sq
    return torch.sqrt(sq.mean())


def rmse(y: torch.Tensor, draws_or_means: torch.Tensor) -> torch.Tensor:
    """sqrt(mean_n (y_n - m_n)^2), m the mean over all leading axes (chain, sample) of draws or predicted means [..., N]
    (evaluation.py:509-512)."""
    m = draws_or_means.reshape(-1, draws_or_means.shape[-1]).mean(dim=0)
    return torch.sqrt(((y.to(m.device, m.dtype) - m) ** 2).mean())


# ---- posterior-predictive moments: the torch restatement of mile_predict_moments (Engine.predict_moments), over raw
# outputs that fit in memory.  The tests' yardstick in fp32, and the CPU fallback of the tools.

def predictive_moments(outputs: torch.Tensor, task: str, return_dropped: bool = False):
    """outputs [..., N, O] raw outputs of all draws (every leading axis is a draw axis) -> [N, W] in the outputs' dtype.
    Regression (W = 3): mean of mu, its population variance over the draws (epistemic), mean of sigma^2 (aleatoric),
    sigma = clip(exp(log sigma), 1e-6, 1e6); columns 1 + 2 are the variance of the equal-weight mixture of the draws'
    Normals.  The variance is the shifted form mean(d^2) - mean(d)^2, d = mu - mean: draws that agree to many digits keep it.
    Classification (W = K + 2): mean softmax probabilities, the entropy of that mean (nats) and the mutual information --
    that entropy minus the mean entropy of the draws, clamped at 0; p = 0 adds 0.
    A draw with a non-finite output on a row is left out of that row; ``return_dropped`` also returns how many, int32 [N].
    A row without a finite draw holds NaN."""
    N, O = outputs.shape[-2], outputs.shape[-1]
    o = outputs.reshape(-1, N, O)
    ok = torch.isfinite(o).all(dim=-1)                                  # [S, N]
    cnt = ok.sum(dim=0)
    w = ok.to(o.dtype)
    n = cnt.to(o.dtype)                                                 # 0 -> 0 / 0 = NaN below
    o = torch.where(ok[..., None], o, torch.zeros_like(o))
    if task in ('regr', 'regression'):
        mu = o[..., 0]
        mean = (mu * w).sum(dim=0) / n
        d = (mu - mean) * w
        var = (d * d).sum(dim=0) / n - (d.sum(dim=0) / n) ** 2
        sig = torch.exp(o[..., 1]).clamp(min=1e-6, max=1e6)
        res = torch.stack([mean, var.clamp(min=0), (sig * sig * w).sum(dim=0) / n], dim=-1)
    else:
        p = torch.softmax(o, dim=-1)
        pm = (p * w[..., None]).sum(dim=0) / n[:, None]
        h_mean = -torch.special.xlogy(pm, pm).sum(dim=-1)
        h_draw = -torch.special.xlogy(p, p).sum(dim=-1)
        mi = (h_mean - (h_draw * w).sum(dim=0) / n).clamp(min=0)
        mi = torch.where(cnt > 0, mi, torch.full_like(mi, float('nan')))     # (clamp keeps NaN; spelled out)
        res = torch.cat([pm, h_mean[:, None], mi[:, None]], dim=-1)
    if return_dropped:
        return res, (o.shape[0] - cnt).to(torch.int32)
    return res


def rmse_from_moments(y: torch.Tensor, moments: torch.Tensor) -> torch.Tensor:
    """sqrt(mean_n (y_n - mean_n)^2) of the predictive mean, column 0 of regression moments [N, 3] (``rmse`` of the draws'
    predicted means, without the draws)."""
    m = moments[:, 0]
    return torch.sqrt(((y.to(m.device, m.dtype).reshape(-1) - m) ** 2).mean())


# ---- exact predictive quantiles and PIT of the ensemble: the torch restatement of mile_mixture_quantiles
# (Engine.mixture_quantiles / predict_quantiles), over raw outputs that fit in memory.  The predictive of row n is the
# equal-weight mixture of the kept draws' Normals, F_n(t) = mean_s Phi((t - mu_sn) / sigma_sn).

def interval_levels(coverages) -> torch.Tensor:
    """The sorted union of ``get_quantiles(c)`` over the nominal coverages, float64 [Q]."""
    lv = torch.cat([get_quantiles(float(c)) for c in coverages])
    return torch.unique(lv, sorted=True)


def _mixture_components(outputs: torch.Tensor):
    """outputs [..., N, 2] -> mu, sigma [S, N] float64 and the mask of kept draws (both outputs finite)."""
    o = outputs.reshape(-1, outputs.shape[-2], 2)
    ok = torch.isfinite(o).all(dim=-1)
    o = torch.where(ok[..., None], o, torch.zeros_like(o)).to(torch.float64)
    return o[..., 0], torch.exp(o[..., 1]).clamp(min=1e-6, max=1e6), ok


def _mixture_cdf(mu, sig, ok, t):
    """mean over the kept draws of Phi((t - mu) / sigma): t [N, Q] -> [N, Q] (0 / 0 = NaN where nothing is kept)."""
    c = torch.special.ndtr((t[None] - mu[..., None]) / sig[..., None]) * ok[..., None]
    return c.sum(dim=0) / ok.sum(dim=0)[:, None]


def mixture_quantiles(outputs: torch.Tensor, levels, return_dropped: bool = False, steps: int = 200):
    """outputs [..., N, 2] raw (mu, log sigma) of all draws (every leading axis is a draw axis), levels [Q] strictly inside
    (0, 1) -> [N, Q] float64: the roots of F_n(t) = p by ``steps`` bisections of the exact bracket, min_s and max_s of
    mu_s + Phi^-1(p) sigma_s.  A draw with a non-finite output on a row is left out of that row; ``return_dropped`` also
    returns how many, int32 [N].  A row with nothing kept holds NaN."""
    mu, sig, ok = _mixture_components(outputs)
    p = torch.as_tensor(levels, dtype=torch.float64, device=mu.device).reshape(-1)
    if p.numel() < 1 or not bool(((p > 0) & (p < 1)).all()):
        raise ValueError('levels must lie strictly inside (0, 1)')
    b = mu[..., None] + torch.special.ndtri(p) * sig[..., None]          # [S, N, Q]
    inf = torch.full_like(b, float('inf'))
    lo = torch.where(ok[..., None], b, inf).amin(dim=0)
    hi = torch.where(ok[..., None], b, -inf).amax(dim=0)
    for _ in range(steps):
        mid = lo + 0.5 * (hi - lo)
        below = _mixture_cdf(mu, sig, ok, mid) < p[None]
        lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
    out = lo + 0.5 * (hi - lo)
    out = torch.where(ok.any(dim=0)[:, None], out, torch.full_like(out, float('nan')))
    if return_dropped:
        return out, (ok.shape[0] - ok.sum(dim=0)).to(torch.int32)
    return out


def mixture_pit(outputs: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """outputs [..., N, 2], y [N] -> the probability integral transform F_n(y_n), float64 [N], with mixture_quantiles'
    leave-out rule."""
    mu, sig, ok = _mixture_components(outputs)
    t = torch.as_tensor(y, device=mu.device).to(torch.float64).reshape(-1, 1)
    return _mixture_cdf(mu, sig, ok, t)[:, 0]


def coverage_from_pit(pit: torch.Tensor, coverages) -> torch.Tensor:
    """Observed coverage of the central intervals from the PIT: mean(|pit - 1/2| <= c / 2) over the rows with a finite PIT,
    float64 [len(coverages)].  y_n lies in the central interval of coverage c exactly when the condition holds."""
    v = pit.to(torch.float64).reshape(-1)
    v = v[torch.isfinite(v)]
    c = torch.as_tensor([float(c) for c in coverages], dtype=torch.float64, device=v.device)
    return ((v[None] - 0.5).abs() <= c[:, None] / 2).to(torch.float64).mean(dim=1)


# ---- the chain-weighted mixture (stacking weights): the torch restatement of mile_mixture_quantiles_weighted
# (Engine.mixture_quantiles_weighted / predict_quantiles_weighted), and the exact composition of per-chain moments and class
# probabilities.  F_n(t) = sum_c (w_c / K_c) sum_{i in c, kept} Phi((t - mu_i) / sigma_i); a chain with w_c = 0 enters no sum,
# a chain with w_c > 0 and nothing kept on a row makes that row NaN.

def chain_weights(weights, C: int) -> torch.Tensor:
    """One chain weight vector, checked as the library checks it (``crps_weights`` for a single vector): [C], every entry finite
    and >= 0, summing to 1 within 1e-9 -> float64 [C] on the host."""
    w = torch.as_tensor(weights, dtype=torch.float64).detach().cpu()
    if w.ndim != 1 or w.shape[0] != C:
        raise ValueError(f'weights must be [{C}], one per chain')
    return crps_weights(w, C)[0]


def _weighted_components(raw: torch.Tensor, weights):
    """raw [C, S, N, 2] -> mu, sigma [C, S, N] float64, omega [C, S, N] = w_c / K_c on the kept draws of the chains that carry
    weight and 0 elsewhere, the kept mask [C, S, N] and the rows [N] on which a weighted chain has nothing kept."""
    if raw.ndim != 4 or raw.shape[-1] != 2:
        raise ValueError('raw must be [C, S, N, 2]')
    w = chain_weights(weights, int(raw.shape[0])).to(raw.device)
    ok = torch.isfinite(raw).all(dim=-1)
    o = torch.where(ok[..., None], raw, torch.zeros_like(raw)).to(torch.float64)
    K = ok.sum(dim=1)                                                       # [C, N]
    use = (w > 0)[:, None] & (K > 0)
    om = torch.where(use, w[:, None] / K.clamp(min=1).to(torch.float64), torch.zeros((), dtype=torch.float64, device=raw.device))
    bad = ((w > 0)[:, None] & (K == 0)).any(dim=0)
    return o[..., 0], torch.exp(o[..., 1]).clamp(min=1e-6, max=1e6), om[:, None, :] * ok, ok, bad


def weighted_mixture_quantiles(raw: torch.Tensor, weights, levels, return_dropped: bool = False, steps: int = 200):
    """raw [C, S, N, 2] (mu, log sigma), weights [C], levels [Q] strictly inside (0, 1) -> [N, Q] float64: the roots of the
    chain-weighted F_n(t) = p by ``steps`` bisections of the exact bracket, min and max of mu_i + Phi^-1(p) sigma_i over the
    components that carry weight.  ``return_dropped`` also returns the draws left out per chain and row, int32 [C, N]."""
    mu, sig, om, ok, bad = _weighted_components(raw, weights)
    p = torch.as_tensor(levels, dtype=torch.float64, device=mu.device).reshape(-1)
    if p.numel() < 1 or not bool(((p > 0) & (p < 1)).all()):
        raise ValueError('levels must lie strictly inside (0, 1)')
    N = mu.shape[-1]
    mu, sig, om = mu.reshape(-1, N), sig.reshape(-1, N), om.reshape(-1, N)
    on = (om > 0)[..., None]
    b = mu[..., None] + torch.special.ndtri(p) * sig[..., None]             # [C * S, N, Q]
    inf = torch.full_like(b, float('inf'))
    lo = torch.where(on, b, inf).amin(dim=0)
    hi = torch.where(on, b, -inf).amax(dim=0)
    for _ in range(steps):
        mid = lo + 0.5 * (hi - lo)
        F = (torch.special.ndtr((mid[None] - mu[..., None]) / sig[..., None]) * om[..., None]).sum(dim=0)
        below = F < p[None]
        lo, hi = torch.where(below, mid, lo), torch.where(below, hi, mid)
    out = lo + 0.5 * (hi - lo)
    out = torch.where(bad[:, None], torch.full_like(out, float('nan')), out)
    if return_dropped:
        return out, (ok.shape[1] - ok.sum(dim=1)).to(torch.int32)
    return out


def weighted_mixture_pit(raw: torch.Tensor, weights, y) -> torch.Tensor:
    """raw [C, S, N, 2], weights [C], y [N] -> the chain-weighted F_n(y_n), float64 [N], NaN where a weighted chain has
    nothing kept."""
    mu, sig, om, _, bad = _weighted_components(raw, weights)
    t = torch.as_tensor(y, device=mu.device).to(torch.float64).reshape(-1)
    F = (torch.special.ndtr((t - mu) / sig) * om).sum(dim=(0, 1))
    return torch.where(bad, torch.full_like(F, float('nan')), F)


def weighted_moments(per_chain: torch.Tensor, kept: torch.Tensor, weights, task: str) -> torch.Tensor:
    """The chain-weighted mixture's moments from the chains' own: per_chain [C, N, W] (``predictive_moments`` /
    Engine.predict_moments of each chain's draws), kept [C, N] (the chain's kept draws on the row), weights [C] -> [N, W]
    float64.  Regression, by the law of total variance with (m_c, e_c, a_c) = per_chain[c]: mean = sum w_c m_c, epistemic =
    sum w_c (e_c + (m_c - mean)^2), aleatoric = sum w_c a_c.  Classification: P = sum w_c P_c, the entropy of P and the mutual
    information H(P) - sum w_c mean-entropy_c (clamped at 0), the chain's mean entropy being H(P_c) - MI_c.  A chain with w_c = 0
    enters no sum; a row on which a chain with w_c > 0 has nothing kept is NaN."""
    C = int(per_chain.shape[0])
    w = chain_weights(weights, C).to(per_chain.device)
    m = per_chain.to(torch.float64)
    on = (w > 0)[:, None] & (kept.to(per_chain.device) > 0)                 # [C, N]
    bad = ((w > 0)[:, None] & ~on).any(dim=0)
    m = torch.where(on[..., None], m, torch.zeros_like(m))
    wc = (w[:, None] * on)[..., None]                                       # [C, N, 1]
    if task in ('regr', 'regression'):
        mean = (wc * m[..., 0:1]).sum(dim=0)                                # [N, 1]
        epi = (wc * (m[..., 1:2] + (m[..., 0:1] - mean) ** 2)).sum(dim=0)
        res = torch.cat([mean, epi, (wc * m[..., 2:3]).sum(dim=0)], dim=-1)
    else:
        K = m.shape[-1] - 2
        P = (wc * m[..., :K]).sum(dim=0)
        h = -torch.special.xlogy(P, P).sum(dim=-1)
        h_c = -torch.special.xlogy(m[..., :K], m[..., :K]).sum(dim=-1) - m[..., K + 1]      # the chain's mean draw entropy
        mi = (h - (wc[..., 0] * h_c).sum(dim=0)).clamp(min=0)
        res = torch.cat([P, h[:, None], mi[:, None]], dim=-1)
    return torch.where(bad[:, None], torch.full_like(res, float('nan')), res)


def weighted_class_probs(probs: torch.Tensor, kept: torch.Tensor, weights):
    """P = sum_c w_c P_c of per-chain mean softmax probabilities probs [C, N, K] with kept [C, N] -> (P [N, K] float64,
    kept [N] int32): kept is 0, and P NaN, on a row where a chain with w_c > 0 has nothing kept, else the kept draws of the
    chains that carry weight -- the pair ``calibration_decide`` takes as one group."""
    C = int(probs.shape[0])
    w = chain_weights(weights, C).to(probs.device)
    kept = kept.to(probs.device)
    on = (w > 0)[:, None] & (kept > 0)
    bad = ((w > 0)[:, None] & ~on).any(dim=0)
    p = torch.where(on[..., None], probs.to(torch.float64), torch.zeros((), dtype=torch.float64, device=probs.device))
    P = ((w[:, None] * on)[..., None] * p).sum(dim=0)
    k = torch.where(bad, torch.zeros_like(kept[0]), (kept * on).sum(dim=0)).to(torch.int32)
    return torch.where(bad[:, None], torch.full_like(P, float('nan')), P), k


# ---- PSIS-LOO and WAIC of the ensemble: the torch restatement of mile_psis_loo (Engine.psis_loo / loo_stream), over a
# pointwise tensor that fits in memory.  The timing tool's yardstick, and what a CPU tensor gets.  All fp64.

_LOG_DBL_MIN = math.log(2.2250738585072014e-308)


def _gpdfit(x: torch.Tensor, budget: int = 1 << 24):
    """Zhang & Stephens' (2009) generalised-Pareto fit of the ascending exceedances x [G, M] -> (khat, sigma, ran) [G]: ``ran``
    is False where the fit does not run (M < 5, x_q <= 0) or gives a non-finite khat or sigma."""
    G, M = x.shape
    nan = torch.full((G,), float('nan'), dtype=x.dtype, device=x.device)
    if M < 5:
        return nan, nan, torch.zeros(G, dtype=torch.bool, device=x.device)
    q = int(math.floor(M / 4 + 0.5))
    m = 30 + int(math.floor(math.sqrt(M)))
    xq, xM = x[:, q - 1], x[:, M - 1]
    j = torch.arange(1, m + 1, dtype=x.dtype, device=x.device)
    b = (1.0 - torch.sqrt(m / (j - 0.5)))[None] / (3.0 * xq)[:, None] + (1.0 / xM)[:, None]        # [G, m]
    k = torch.empty_like(b)
    step = max(1, budget // (m * M))
    for g0 in range(0, G, step):                                        # [g, m, M] at a time
        k[g0:g0 + step] = torch.log1p(-b[g0:g0 + step, :, None] * x[g0:g0 + step, None, :]).mean(dim=-1)
    L = M * (torch.log(-b / k) - k - 1.0)
    w = 1.0 / torch.exp(L[:, :, None] - L[:, None, :]).sum(dim=1)       # w_j = 1 / sum_i exp(L_i - L_j); inf -> 0
    bb = (b * w).sum(dim=1)
    kk = torch.log1p(-bb[:, None] * x).mean(dim=1)
    sigma = -kk / bb
    khat = (M * kk + 5.0) / (M + 10.0)
    ran = (xq > 0) & torch.isfinite(khat) & torch.isfinite(sigma)
    return torch.where(ran, khat, nan), torch.where(ran, sigma, nan), ran


def psis_loo(loglik: torch.Tensor, r_eff: float = 1.0) -> dict:
    """loglik [..., N] = log p(y_n | x_n, theta_s) (every leading axis is a draw axis) -> per-row fp64 tensors ``lppd``,
    ``p_waic``, ``elpd_loo``, ``khat`` [N] and ``dropped`` [N] int32: Pareto-smoothed importance-sampling leave-one-out
    (Vehtari, Gelman & Gabry 2017; Vehtari et al. 2024) and WAIC.  A draw whose value on a row is NaN or +-inf is left out of
    that row and counted; with S_n kept, lppd = logsumexp l - log S_n, p_waic the ddof-1 variance of l, and the
    M = ceil(min(S_n / 5, 3 sqrt(S_n / r_eff))) largest ratios r = -l - max(-l) are replaced by the quantiles of the
    generalised Pareto fitted to them (no fit and khat = NaN when M < 5 or the tail is degenerate), capped at 0 and
    normalised; elpd_loo = logsumexp(lw + l).  A row with fewer than two kept draws holds NaN."""
    if not (math.isfinite(r_eff) and r_eff > 0):
        raise ValueError('r_eff must be finite and positive')
    N = loglik.shape[-1]
    l = loglik.reshape(-1, N).t().to(torch.float64)                     # [N, S]
    S, dev = l.shape[1], l.device
    ok = torch.isfinite(l)
    Sn = ok.sum(dim=1)
    out = {k: torch.full((N,), float('nan'), dtype=torch.float64, device=dev) for k in ('lppd', 'p_waic', 'elpd_loo', 'khat')}
    out['dropped'] = (S - Sn).to(torch.int32)
    neg = torch.where(ok, -l, torch.full_like(l, -float('inf')))
    rs, idx = torch.sort(neg, dim=1)                                    # ascending; the dropped draws come first
    ls = torch.gather(l, 1, idx)
    del neg, idx, l, ok
    for sn in torch.unique(Sn).tolist():
        if sn < 2:
            continue
        rows = torch.nonzero(Sn == sn).reshape(-1)
        lg = ls[rows, S - sn:]                                          # the kept draws, l descending
        rg = rs[rows, S - sn:]
        rg = rg - rg[:, -1:]                                            # r = -l - max(-l), ascending
        out['lppd'][rows] = torch.logsumexp(lg, dim=1) - math.log(sn)
        out['p_waic'][rows] = ((lg - lg.mean(dim=1, keepdim=True)) ** 2).sum(dim=1) / (sn - 1)
        M = int(math.ceil(min(sn / 5.0, 3.0 * math.sqrt(sn / r_eff))))
        cut = rg[:, sn - M - 1].clamp(min=_LOG_DBL_MIN)
        ec = torch.exp(cut)
        tail = rg[:, sn - M:]
        khat, sigma, ran = _gpdfit(torch.exp(tail) - ec[:, None])
        p = (torch.arange(1, M + 1, dtype=torch.float64, device=dev) - 0.5) / M
        lp = torch.log1p(-p)[None]
        qv = torch.where((khat == 0)[:, None], -sigma[:, None] * lp, sigma[:, None] * torch.expm1(-khat[:, None] * lp) / khat[:, None])
        lw = torch.cat([rg[:, :sn - M], torch.where(ran[:, None], torch.log(qv + ec[:, None]), tail)], dim=1).clamp(max=0.0)
        lw = lw - torch.logsumexp(lw, dim=1, keepdim=True)
        out['elpd_loo'][rows] = torch.logsumexp(lw + lg, dim=1)
        out['khat'][rows] = khat
    return out


def loo_summary(rows: dict) -> dict:
    """The totals of per-row PSIS-LOO / WAIC arrays (``psis_loo``, Engine.psis_loo or Engine.loo_stream), on the host in fp64:
    ``elpd_loo`` = sum_n elpd_loo_n with ``se_elpd_loo`` = sqrt(N var_n) (var with divisor N - 1, as the loo package) and
    ``p_loo`` = sum_n (lppd_n - elpd_loo_n); ``elpd_waic`` = sum_n (lppd_n - p_waic_n) with ``se_elpd_waic`` and ``p_waic``;
    ``lppd_sum``; and the diagnostics ``n_khat_above_0.7`` (finite khat only), ``n_khat_nofit`` (NaN khat) and
    ``n_p_waic_above_0.4``.  A NaN row (fewer than two kept draws) makes the sums NaN."""
    import numpy as np
    a = {k: (rows[k].detach().cpu().numpy() if isinstance(rows[k], torch.Tensor) else np.asarray(rows[k])).astype(np.float64).reshape(-1)
         for k in ('lppd', 'p_waic', 'elpd_loo', 'khat')}
    N = a['lppd'].shape[0]
    se = lambda v: float(np.sqrt(N * np.var(v, ddof=1))) if N > 1 else float('nan')
    waic = a['lppd'] - a['p_waic']
    khat = a['khat']
    with np.errstate(invalid='ignore'):
        return {'elpd_loo': float(a['elpd_loo'].sum()), 'se_elpd_loo': se(a['elpd_loo']), 'p_loo': float((a['lppd'] - a['elpd_loo']).sum()),
                'elpd_waic': float(waic.sum()), 'se_elpd_waic': se(waic), 'p_waic': float(a['p_waic'].sum()),
                'lppd_sum': float(a['lppd'].sum()),
                'n_khat_above_0.7': int((khat[np.isfinite(khat)] > 0.7).sum()), 'n_khat_nofit': int(np.isnan(khat).sum()),
                'n_p_waic_above_0.4': int((a['p_waic'] > 0.4).sum())}


# ---- PSIS-LOO expectations and LOO-PIT: the torch restatement of mile_psis_expect (Engine.psis_expect / loo_predict_stream)
# over tensors that fit in memory, the predictive columns, and what evaluate.py --loo-predict reports.  All fp64.

def psis_weights_dense(loglik: torch.Tensor, r_eff: float = 1.0) -> dict:
    """loglik [..., N] -> ``weights`` [N, S] fp64, the smoothed, capped and normalised PSIS weights of ``psis_loo`` in draw
    order (0 for a dropped draw), with the tie rule: draws of a row with equal l share the mean of their weights, so the
    weights are a function of the multiset of a row's draws.  Also ``ess_w`` = 1 / sum w^2, ``khat``, ``elpd_loo`` [N] and
    ``dropped`` [N] int32.  A row with fewer than two kept draws holds NaN (its weights too)."""
    if not (math.isfinite(r_eff) and r_eff > 0):
        raise ValueError('r_eff must be finite and positive')
    N = loglik.shape[-1]
    l = loglik.reshape(-1, N).t().to(torch.float64)                     # [N, S]
    S, dev = l.shape[1], l.device
    ok = torch.isfinite(l)
    Sn = ok.sum(dim=1)
    nan = float('nan')
    out = {k: torch.full((N,), nan, dtype=torch.float64, device=dev) for k in ('ess_w', 'khat', 'elpd_loo')}
    out['dropped'] = (S - Sn).to(torch.int32)
    neg = torch.where(ok, -l, torch.full_like(l, -float('inf')))
    rs, idx = torch.sort(neg, dim=1, stable=True)                       # ascending; the dropped draws come first
    ls = torch.gather(l, 1, idx)
    ws = torch.zeros_like(l)                                            # the weights in sorted order
    for sn in torch.unique(Sn).tolist():
        rows = torch.nonzero(Sn == sn).reshape(-1)
        if sn < 2:
            ws[rows] = nan
            continue
        lg = ls[rows, S - sn:]                                          # the kept draws, l descending
        rg = rs[rows, S - sn:]
        rg = rg - rg[:, -1:]                                            # r = -l - max(-l), ascending
        M = int(math.ceil(min(sn / 5.0, 3.0 * math.sqrt(sn / r_eff))))
        cut = rg[:, sn - M - 1].clamp(min=_LOG_DBL_MIN)
        ec = torch.exp(cut)
        tail = rg[:, sn - M:]
        khat, sigma, ran = _gpdfit(torch.exp(tail) - ec[:, None])
        p = (torch.arange(1, M + 1, dtype=torch.float64, device=dev) - 0.5) / M
        lp = torch.log1p(-p)[None]
        qv = torch.where((khat == 0)[:, None], -sigma[:, None] * lp, sigma[:, None] * torch.expm1(-khat[:, None] * lp) / khat[:, None])
        lw = torch.cat([rg[:, :sn - M], torch.where(ran[:, None], torch.log(qv + ec[:, None]), tail)], dim=1).clamp(max=0.0)
        lw = lw - torch.logsumexp(lw, dim=1, keepdim=True)
        out['elpd_loo'][rows] = torch.logsumexp(lw + lg, dim=1)
        out['khat'][rows] = khat
        w = torch.exp(lw)
        G = rows.numel()                                                # the mean over every run of equal l (adjacent once sorted)
        first = torch.cat([torch.ones((G, 1), dtype=torch.bool, device=dev), lg[:, 1:] != lg[:, :-1]], dim=1)
        run = (torch.cumsum(first.reshape(-1).to(torch.int64), 0) - 1)  # rows start a run: ids never cross a row
        tot = torch.zeros(int(run[-1]) + 1, dtype=torch.float64, device=dev).index_add_(0, run, w.reshape(-1))
        cnt = torch.zeros_like(tot).index_add_(0, run, torch.ones_like(w).reshape(-1))
        w = (tot / cnt)[run].reshape(G, sn)
        out['ess_w'][rows] = 1.0 / (w * w).sum(dim=1)
        ws[rows, S - sn:] = w
    out['weights'] = torch.zeros_like(l).scatter_(1, idx, ws)
    return out


def psis_expect_dense(loglik: torch.Tensor, values: torch.Tensor, r_eff: float = 1.0, return_weights: bool = False) -> dict:
    """The torch form of Engine.psis_expect: loglik [S, N] and values [S, N, Q] (any float dtype, read as fp64) -> ``expect``
    [N, Q] = sum_s w_s h_q(s, n) with ``psis_weights_dense``'s weights, ``posterior`` [N, Q] the mean over the kept draws,
    ``ess_w``, ``khat``, ``elpd_loo`` [N], ``dropped`` [N] (and ``weights`` [N, S]).  The values of a dropped draw enter no
    sum; a non-finite value of a kept draw propagates by IEEE rules; a row with fewer than two kept draws holds NaN."""
    out = psis_weights_dense(loglik, r_eff)
    W = out['weights'] if return_weights else out.pop('weights')        # [N, S]
    N, S = W.shape
    v = values.reshape(S, N, -1).to(torch.float64).permute(1, 0, 2)     # [N, S, Q]
    ok = torch.isfinite(loglik.reshape(S, N).t())
    v = torch.where(ok[..., None], v, torch.zeros_like(v))
    Sn = ok.sum(dim=1)
    few = (Sn < 2)[:, None]
    nan = torch.full((), float('nan'), dtype=torch.float64, device=W.device)
    out['expect'] = torch.where(few, nan, (torch.where(ok, W, torch.zeros_like(W))[..., None] * v).sum(dim=1))
    out['posterior'] = torch.where(few, nan, v.sum(dim=1) / Sn.clamp(min=1)[:, None].to(torch.float64))
    return out


def loo_predict_columns(raw: torch.Tensor, y, task: str) -> torch.Tensor:
    """The predictive columns of mile_loo_predict_stream from raw outputs raw [..., N, O] (Engine.predict), fp64 [..., N, Q]:
    regression (mu, log sigma) -> (mu, mu^2, sigma^2, Phi((y - mu) / sigma)) with sigma = exp(log sigma) clipped to
    [1e-6, 1e6]; classification -> softmax(raw)."""
    z = raw.to(torch.float64)
    if task == 'regr':
        mu = z[..., 0]
        es = torch.exp(z[..., 1])
        sig = torch.where(torch.isnan(es), es, es.clamp(1e-6, 1e6))
        yt = torch.as_tensor(y, device=z.device).to(torch.float64)
        return torch.stack([mu, mu * mu, sig * sig, 0.5 * torch.erfc(-((yt - mu) / sig) * 0.70710678118654752440)], dim=-1)
    m = z.max(dim=-1, keepdim=True).values
    return torch.exp(z - (m + torch.log(torch.exp(z - m).sum(dim=-1, keepdim=True))))


def loo_predict(eng, samples, x, y, r_eff: float = 1.0, max_draws_per_pass: int = 0, max_rows_per_tile: int = 0, dense: bool = False) -> dict:
    """Leave-one-out predictions of the ensemble on the rows (x, y) it conditioned on: Engine.loo_predict_stream where the
    library's limits allow (2 <= S <= 2^20 pooled draws, a tail of at most 4096, (mu, log sigma) or at most 64 classes),
    otherwise -- or with ``dense`` -- ``psis_expect_dense`` of Engine.pointwise_loglik's tensor and the columns of
    Engine.predict's.  ``samples`` [..., d]: every leading axis is a draw axis."""
    th = torch.as_tensor(samples).reshape(-1, eng.d)
    S = int(th.shape[0])
    task = eng.spec.task
    fits = 2 <= S <= (1 << 20) and math.ceil(min(S / 5.0, 3.0 * math.sqrt(S / r_eff))) <= 4096 and eng.loo_predict_stream_workspace(S, len(x)) > 0
    if fits and not dense:
        return eng.loo_predict_stream(th, x, y, r_eff=r_eff, max_draws_per_pass=max_draws_per_pass, max_rows_per_tile=max_rows_per_tile)
    ll = eng.pointwise_loglik(th, x, y)
    cols = loo_predict_columns(eng.predict(th, x), torch.as_tensor(y).to(ll.device), 'regr' if task == 'regr' else 'class')
    return psis_expect_dense(ll, cols, r_eff)


def loo_predict_summary(rows: dict, y, task: str, coverages=(0.5, 0.75, 0.9, 0.95), n_bins: int = 15) -> dict:
    """What a per-row LOO prediction (``loo_predict``, Engine.loo_predict_stream or ``psis_expect_dense`` of the predictive
    columns) says, on the host in fp64; every key once from ``expect`` and once, with ``_insample``, from ``posterior``.
    Regression (columns mu, mu^2, sigma^2, PIT): ``rmse`` and ``r2`` of the predictive mean, ``var_epistemic`` = mean_n
    (E[mu^2] - E[mu]^2), ``var_aleatoric`` = mean_n E[sigma^2], ``coverage_<c>`` of the central intervals from the PIT
    (``coverage_from_pit``) and their ``cal_error``.  Classification (columns: the class probabilities): ``accuracy``,
    ``brier``, ``nll``, ``ece`` and ``mce`` (``calibration_decide``); the LOO ``nll`` is -mean_n elpd_loo.  Rows with a
    non-finite prediction are left out and counted in ``n_rows_nan``.  Then the diagnostics of the weights:
    ``khat_above_0.7_share`` (of the rows with a fitted tail), ``khat_nofit``, ``ess_w_min``, ``ess_w_median``, ``n_rows``,
    ``dropped``."""
    f = lambda k: torch.as_tensor(rows[k]).detach().cpu().to(torch.float64)
    yt = torch.as_tensor(y).detach().cpu().reshape(-1)
    N = int(yt.shape[0])
    cov = [float(c) for c in coverages]
    out = {}
    for tag, E in (('', f('expect')), ('_insample', f('posterior'))):
        E = E.reshape(N, -1)
        good = torch.isfinite(E).all(dim=1)
        if task == 'regr':
            yv = yt.to(torch.float64)[good]
            mean, m2, alea, pit = (E[good, i] for i in range(4))
            sq = (yv - mean) ** 2
            out['rmse' + tag] = float(torch.sqrt(sq.mean()))
            out['r2' + tag] = float(1.0 - sq.sum() / ((yv - yv.mean()) ** 2).sum())
            out['var_epistemic' + tag] = float((m2 - mean * mean).mean())
            out['var_aleatoric' + tag] = float(alea.mean())
            obs = coverage_from_pit(pit, cov)
            for c, v in zip(cov, obs):
                out[f'coverage_{c}{tag}'] = float(v)
            out['cal_error' + tag] = float(calibration_error(cov, obs))
        else:
            dec = calibration_decide(E[None], good[None].to(torch.int32), yt, cov, n_bins)
            s = calibration_summary({'totals': dec['totals'], 'bins': dec['bins'], 'coverages': cov})[0]
            for k_out, k_in in (('accuracy', 'acc'), ('brier', 'brier'), ('nll', 'nll'), ('ece', 'ece'), ('mce', 'mce')):
                out[k_out + tag] = s[k_in]
        if not tag:
            out['n_rows_nan'] = int((~good).sum())
    if task != 'regr':
        el = f('elpd_loo')
        out['nll'] = float(-el.mean())
    khat, ess = f('khat'), f('ess_w')
    fitted = torch.isfinite(khat)
    out['khat_above_0.7_share'] = float((khat[fitted] > 0.7).to(torch.float64).mean()) if bool(fitted.any()) else float('nan')
    out['khat_nofit'] = int((~fitted).sum())
    fin = ess[torch.isfinite(ess)]
    out['ess_w_min'] = float(fin.min()) if fin.numel() else float('nan')
    out['ess_w_median'] = float(fin.median()) if fin.numel() else float('nan')
    out['n_rows'] = N
    out['dropped'] = int(torch.as_tensor(rows['dropped']).sum())
    return out


# ---- prediction sets and calibration of the classification ensemble: the torch restatement of mile_calibration
# (Engine.calibration / calibration_stream) over logits that fit in memory.  The fallback for K > 64 and the tools' yardstick.

def calibration_decide(probs: torch.Tensor, kept: torch.Tensor, y, coverages, n_bins: int = 15) -> dict:
    """Group probabilities probs [G, N, K] fp64 (the last group is the ensemble) and kept [G, N] -> every discrete and summed
    output of mile_calibration: ``order`` [N, K], ``set_size`` [N, Q] int32 of the ensemble, and with labels ``y`` [N] ``rank``
    [N] int32, ``totals`` [G, 5 + 2 Q] and ``bins`` [G, n_bins, 3] fp64 (include/mile_hip.h states the definition).  The
    cumulative sum that sizes a set is sequential, as in the library."""
    G, N, K = probs.shape
    dev = probs.device
    cov = torch.as_tensor(coverages, dtype=torch.float64, device=dev).reshape(-1)
    Q = int(cov.numel())
    empty = kept.to(dev) == 0                                            # [G, N]
    P = torch.where(empty[..., None], torch.zeros_like(probs), probs)
    order = torch.argsort(-P, dim=-1, stable=True)                       # ties to the lower class index
    order = torch.where(empty[..., None], torch.arange(K, device=dev).expand(G, N, K), order)
    Ps = torch.gather(P, -1, order)
    size = torch.zeros((G, N, Q), dtype=torch.int32, device=dev)
    cum = torch.zeros((G, N), dtype=torch.float64, device=dev)
    for i in range(K):
        cum = cum + Ps[..., i]
        hit = (cum[..., None] >= cov) & (size == 0)
        size = torch.where(hit, torch.full_like(size, i + 1), size)
    size = torch.where(size == 0, torch.full_like(size, K), size)
    size = torch.where(empty[..., None], torch.zeros_like(size), size)
    out = {'order': order[-1].to(torch.int32), 'set_size': size[-1]}
    if y is None:
        return out
    yl = torch.as_tensor(y, device=dev).to(torch.int64).reshape(-1)
    bad = (yl < 0) | (yl >= K)
    ys = torch.where(bad, torch.zeros_like(yl), yl)
    rank = (order == ys[None, :, None]).to(torch.int32).argmax(dim=-1).to(torch.int32) + 1
    rank = torch.where(bad[None] | empty, torch.zeros_like(rank), rank)
    valid = ~empty & ~bad[None]
    onehot = torch.nn.functional.one_hot(ys, K).to(torch.float64)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    brier = torch.where(valid, ((P - onehot[None]) ** 2).sum(dim=-1), zero)
    nll = torch.where(valid, -torch.log(torch.gather(P, -1, ys[None, :, None].expand(G, N, 1))[..., 0]), zero)
    conf = Ps[..., 0]
    correct = (rank == 1) & valid
    f = lambda t: t.to(torch.float64)
    covered = (rank[..., None] <= size) & valid[..., None]
    totals = torch.cat([torch.stack([f(valid).sum(1), f(correct).sum(1), brier.sum(1), nll.sum(1), f(bad[None] & ~empty).sum(1)], dim=1),
                        f(covered).sum(1), (f(size) * f(valid)[..., None]).sum(1)], dim=1)
    b = torch.clamp(torch.floor(conf * n_bins).to(torch.int64), max=n_bins - 1)
    b = torch.where(valid, b, torch.zeros_like(b))
    bins = torch.zeros((G, n_bins, 3), dtype=torch.float64, device=dev)
    for j, v in enumerate((f(valid), torch.where(valid, conf, zero), f(correct))):
        bins[..., j].scatter_add_(1, b, v)
    out.update(rank=rank[-1], totals=totals, bins=bins)
    return out


def classification_calibration(raw: torch.Tensor, y=None, coverages=(0.5, 0.75, 0.9, 0.95), n_bins: int = 15,
                               budget: int = 1 << 28) -> dict:
    """The plain-torch form of Engine.calibration: logits raw [C, S, N, K] (any float dtype; the arithmetic is fp64) -> the same
    dict -- ``coverages``, ``probs`` [C + 1, N, K] fp64, ``kept`` [C + 1, N] int32, ``order``, ``set_size``, and with ``y``
    ``rank``, ``totals``, ``bins``.  A draw is kept on a row iff all its logits there are finite; a group's probabilities are
    the mean softmax of its kept draws (the ensemble: all chains' draws), NaN with nothing kept.  No bound on K.  The draws
    go through in slices of about ``budget`` bytes."""
    C_, S_, N, K = raw.shape
    dev = raw.device
    sums = torch.zeros((C_, N, K), dtype=torch.float64, device=dev)
    cnt = torch.zeros((C_, N), dtype=torch.int64, device=dev)
    step = max(1, budget // max(1, C_ * N * K * 8 * 4))
    for s0 in range(0, S_, step):
        z = raw[:, s0:s0 + step]
        ok = torch.isfinite(z).all(dim=-1)                               # [C, s, N]
        z = torch.where(ok[..., None], z, torch.zeros_like(z)).to(torch.float64)
        e = torch.exp(z - z.max(dim=-1, keepdim=True).values)
        p = e / e.sum(dim=-1, keepdim=True)
        sums += (p * ok[..., None]).sum(dim=1)
        cnt += ok.sum(dim=1)
    kept = torch.cat([cnt, cnt.sum(dim=0, keepdim=True)])
    tot = torch.cat([sums, sums.sum(dim=0, keepdim=True)])
    probs = torch.where(kept[..., None] > 0, tot / kept[..., None].to(torch.float64), torch.full_like(tot, float('nan')))
    out = {'coverages': torch.as_tensor(coverages, dtype=torch.float64, device=dev).reshape(-1), 'probs': probs,
           'kept': kept.to(torch.int32)}
    out.update(calibration_decide(probs, kept, y, out['coverages'], n_bins))
    return out


def calibration_summary(result: dict) -> list:
    """Per group (each chain, then the ensemble) of a calibration result's ``totals``, ``bins`` and ``coverages``: ``rows``,
    ``acc``, ``brier``, ``nll`` (means over the rows counted), ``ece`` = sum_b |sum correct_b - sum conf_b| / rows, ``mce`` =
    the largest |mean correct_b - mean conf_b| of a non-empty bin, ``coverage_<c>`` and ``set_size_<c>`` (share of rows whose
    label is in the set, mean set size) and ``cal_error`` = ``calibration_error`` of the coverages.  Highest-probability sets
    reach their level by construction, so that error is one-sided.  A group without rows holds NaN."""
    tot = torch.as_tensor(result['totals']).detach().double().cpu()
    bins = torch.as_tensor(result['bins']).detach().double().cpu()
    cov = [float(v) for v in torch.as_tensor(result['coverages'], dtype=torch.float64).reshape(-1)]
    Q = len(cov)
    res = []
    for g in range(tot.shape[0]):
        rows = float(tot[g, 0])
        nan = float('nan')
        d = {'rows': int(rows), 'bad_labels': int(tot[g, 4])}
        for i, k in enumerate(('acc', 'brier', 'nll')):
            d[k] = float(tot[g, 1 + i]) / rows if rows else nan
        gap = (bins[g, :, 2] - bins[g, :, 1]).abs()
        full = bins[g, :, 0] > 0
        d['ece'] = float(gap.sum()) / rows if rows else nan
        d['mce'] = float((gap[full] / bins[g, full, 0]).max()) if bool(full.any()) else nan
        obs = [float(tot[g, 5 + q]) / rows if rows else nan for q in range(Q)]
        for q, c in enumerate(cov):
            d[f'coverage_{c}'] = obs[q]
            d[f'set_size_{c}'] = float(tot[g, 5 + Q + q]) / rows if rows else nan
        d['cal_error'] = float(calibration_error(cov, obs).item())
        res.append(d)
    return res


# ---- stacking of chains that do not mix (Yao, Vehtari, Simpson & Gelman 2018; Yao, Vehtari & Gelman 2022): the torch restatement
# of mile_stack_eval (Engine.stack_eval), the solver for the weights on either of them, and what evaluate.py --stacking reports.

_STACK_OUTPUTS = ('score', 'row_score', 'grad', 'hess', 'used')


def stack_eval_dense(lpd: torch.Tensor, w, outputs=('score', 'grad', 'hess', 'used'), max_rows_per_tile: int = 0) -> dict:
    """lpd [C, N] and w [C] (entries >= 0) -> the ``outputs`` asked for among ``score`` [], ``row_score`` [N], ``grad`` [C],
    ``hess`` [C, C] (fp64) and ``used`` [] int64, on lpd's device: the log score of the w-weighted mixture of the chains'
    pointwise predictive densities, its gradient in w and the Gram matrix of the responsibilities (the negative Hessian).  A row
    with a NaN or +inf entry, or with no entry above -inf, is left out (NaN in ``row_score``) and ``used`` counts the rest; with
    m_n = max_c lpd_cn, e = exp(lpd - m), mix_n = sum_c w_c e_cn and R = e / mix: row_score = m + log mix, score its mean,
    grad_c the mean of R_cn, hess_ab the mean of R_an R_bn over the used rows.  A used row with mix_n = 0 makes the score -inf.
    The any-device form of Engine.stack_eval, with its signature (``max_rows_per_tile`` means nothing here)."""
    outputs = tuple(outputs)
    if not outputs or any(k not in _STACK_OUTPUTS for k in outputs):
        raise ValueError(f'outputs: a non-empty choice of {_STACK_OUTPUTS}')
    l = torch.as_tensor(lpd).to(torch.float64)
    if l.ndim != 2:
        raise ValueError('lpd must be [C, N]')
    w = torch.as_tensor(w).to(device=l.device, dtype=torch.float64).reshape(-1)
    if w.shape != (l.shape[0],):
        raise ValueError('w must be [C]')
    m = torch.where(torch.isnan(l), torch.full_like(l, -float('inf')), l).max(dim=0).values
    ok = ~(torch.isnan(l) | (l == float('inf'))).any(dim=0) & (m > -float('inf'))
    lu, mu = l[:, ok], m[ok]
    used = int(lu.shape[1])
    e = torch.exp(lu - mu[None])
    mix = (w[:, None] * e).sum(dim=0)
    res = {}
    if 'row_score' in outputs:
        res['row_score'] = torch.full((l.shape[1],), float('nan'), dtype=torch.float64, device=l.device)
        res['row_score'][ok] = mu + torch.log(mix)
    if 'used' in outputs:
        res['used'] = torch.tensor(used, dtype=torch.int64, device=l.device)
    if 'score' in outputs:
        res['score'] = (mu + torch.log(mix)).sum() / used if used else torch.tensor(float('nan'), dtype=torch.float64, device=l.device)
    if 'grad' in outputs or 'hess' in outputs:
        R = e / mix[None]
        if 'grad' in outputs:
            res['grad'] = R.sum(dim=1) / used if used else torch.full_like(w, float('nan'))
        if 'hess' in outputs:
            h = (R @ R.t()) / used if used else torch.full((l.shape[0],) * 2, float('nan'), dtype=torch.float64, device=l.device)
            res['hess'] = torch.tril(h) + torch.tril(h, -1).t()
    return res


def _stack_qp(H, g, w):
    """min over y >= 0 of 1/2 y'Hy + (1 - g - Hw)'y by an active-set method from y = w (fp64 NumPy): the free set starts as the
    positive entries, a ridge 1e-12 I steadies the free block, a negative component of the free block's solution moves y to
    the boundary and binds the blocking entry, and at a feasible solution the bound entry with the most negative multiplier
    is released.  (Kim, Carbonetto, Stephens & Anitescu 2020, the subproblem of mix-SQP.)"""
    import numpy as np
    C = w.shape[0]
    q = 1.0 - g - H @ w
    y = w.copy()
    free = y > 0
    for _ in range(4 * C + 16):
        F = np.flatnonzero(free)
        z = np.zeros(C)
        if F.size:
            z[F] = np.linalg.solve(H[np.ix_(F, F)] + 1e-12 * np.eye(F.size), -q[F])
        if F.size and (z[F] < 0).any():
            d = z - y
            neg = F[z[F] < 0]
            ratio = y[neg] / np.maximum(y[neg] - z[neg], 1e-300)
            k = int(np.argmin(ratio))
            y = np.maximum(y + float(ratio[k]) * d, 0.0)
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


def stacking_weights(lpd, tol: float = 1e-8, max_iter: int = 50, eval=None, w0=None) -> dict:
    """The stacking weights of chains with pointwise leave-one-out log densities lpd [C, N] (Engine.chain_loo_stream's
    ``elpd_loo``): the w on the simplex that maximise the mean log score of the weighted mixture, by Newton steps on
    phi(w) = -score(w) + sum(w) over w >= 0 (whose minimiser sums to 1), each from the active-set QP of ``_stack_qp`` on the
    gradient and Hessian that ``eval`` returns -- Engine.stack_eval for the kernels, None for ``stack_eval_dense`` -- followed
    by a backtracking line search (t halved from 1, score-only evaluations of w + t p clipped at 0, Armijo constant 1e-4 on phi,
    a non-finite score rejects the step) and a renormalisation to sum 1.  From w0 (None: 1 / C).
    Stops when gap = max_c grad_c - 1 <= tol: by concavity score(w*) - score(w) <= gap, so ``gap`` certifies the value returned.
    Returns ``w`` [C] (fp64 NumPy), ``score``, ``gap``, ``iterations`` (Newton steps), ``score_evals`` (line-search
    evaluations), ``converged`` and ``used``; reaching ``max_iter``, or a step the line search cannot place, returns
    ``converged`` False with the gap of the last evaluation, never an exception."""
    import numpy as np
    ev = stack_eval_dense if eval is None else eval
    if not isinstance(lpd, torch.Tensor):
        lpd = torch.as_tensor(np.asarray(lpd, dtype=np.float64))
    C = int(lpd.shape[0])
    w = np.full(C, 1.0 / C) if w0 is None else np.asarray(w0, dtype=np.float64).reshape(-1).copy()
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)
    iters = score_evals = 0
    while True:
        r = ev(lpd, torch.from_numpy(w), outputs=('score', 'grad', 'hess', 'used'))
        score, used = float(r['score']), int(r['used'])
        if not math.isfinite(score):
            return {'w': w, 'score': score, 'gap': float('inf'), 'iterations': iters, 'score_evals': score_evals, 'converged': False,
                    'used': used}
        g, H = host(r['grad']), host(r['hess'])
        gap = float(g.max() - 1.0)
        if gap <= tol or iters >= max_iter:
            return {'w': w, 'score': score, 'gap': gap, 'iterations': iters, 'score_evals': score_evals, 'converged': gap <= tol,
                    'used': used}
        p = _stack_qp(H, g, w) - w
        slope = float((1.0 - g) @ p)
        phi0 = -score + w.sum()
        t, placed = 1.0, False
        for _ in range(60):
            wt = np.maximum(w + t * p, 0.0)
            st = float(ev(lpd, torch.from_numpy(wt), outputs=('score',))['score'])
            score_evals += 1
            if math.isfinite(st) and -st + wt.sum() <= phi0 + 1e-4 * t * slope:
                placed = True
                break
            t *= 0.5
        if not placed or not (wt.sum() > 0) or np.array_equal(wt / wt.sum(), w):
            return {'w': w, 'score': score, 'gap': gap, 'iterations': iters, 'score_evals': score_evals, 'converged': False,
                    'used': used}
        w = wt / wt.sum()
        iters += 1


def weighted_lppd(lpd_test, w, eval=None) -> float:
    """The mean over the used rows of log sum_c w_c exp(lpd_test[c, n]): the score of ``stack_eval_dense`` (``eval`` as for
    ``stacking_weights``) at fixed w.  With w = 1 / C and per-chain LPPD rows it is the ensemble's LPPD."""
    ev = stack_eval_dense if eval is None else eval
    return float(ev(lpd_test, torch.as_tensor(w, dtype=torch.float64), outputs=('score',))['score'])


def stacking_summary(rows: dict) -> dict:
    """Per chain, from per-chain PSIS-LOO arrays [C, N] (Engine.chain_loo_stream), on the host in fp64: ``chain_elpd_loo`` the
    sum over the rows of elpd_loo (NaN rows left out, ``chain_rows_nan`` counting them) and ``chain_khat_bad`` the rows with a
    finite khat > 0.7; ``n_rows``."""
    import numpy as np
    a = {k: (rows[k].detach().cpu().numpy() if isinstance(rows[k], torch.Tensor) else np.asarray(rows[k])).astype(np.float64)
         for k in ('elpd_loo', 'khat')}
    with np.errstate(invalid='ignore'):
        return {'chain_elpd_loo': [float(v) for v in np.nansum(a['elpd_loo'], axis=1)],
                'chain_rows_nan': [int(v) for v in np.isnan(a['elpd_loo']).sum(axis=1)],
                'chain_khat_bad': [int(v) for v in (np.isfinite(a['khat']) & (a['khat'] > 0.7)).sum(axis=1)],
                'n_rows': int(a['elpd_loo'].shape[1])}


CRPS_OUTPUTS = ('crps_chain', 'spread_chain', 'crps_mix', 'spread_mix', 'gram', 'dropped')
CRPS_MAX_WEIGHTS = 8


def crps_weights(weights, C: int) -> torch.Tensor:
    """Chain weight vectors for the CRPS of a weighted mixture, checked as the library checks them: None -> [0, C]; [C] or
    [n_w, C] with n_w <= 8, every entry finite and >= 0, every vector summing to 1 within 1e-9 -> float64 [n_w, C] on the host."""
    if weights is None:
        return torch.zeros((0, C), dtype=torch.float64)
    w = torch.as_tensor(weights, dtype=torch.float64).detach().cpu()        # (a list goes straight to fp64, not through fp32)
    if w.ndim == 1:
        w = w[None]
    if w.ndim != 2 or w.shape[1] != C:
        raise ValueError(f'weights must be [{C}] or [n_w, {C}]')
    if w.shape[0] > CRPS_MAX_WEIGHTS:
        raise ValueError(f'weights: at most {CRPS_MAX_WEIGHTS} vectors')
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError('weights must be finite and >= 0')
    if bool(((w.sum(dim=1) - 1.0).abs() > 1e-9).any()):
        raise ValueError('every weight vector must sum to 1 (within 1e-9)')
    return w.contiguous()


def crps_thin_stride(C: int, S: int, max_draws: int) -> int:
    """k = ceil(C * S / max_draws), at least 1: every chain keeps its draws j = 0 mod k (``samples[:, ::k]``), so at most
    about ``max_draws`` draws enter the CRPS's pair sums."""
    if max_draws < 1:
        raise ValueError('max_draws must be >= 1')
    return max(1, -(-(int(C) * int(S)) // int(max_draws)))


def _abs_normal_mean(d: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """A(d, v) = E|N(d, v)| = d erf(d / sqrt(2 v)) + sqrt(2 v / pi) exp(-d^2 / (2 v))."""
    return d * torch.erf(d / torch.sqrt(2.0 * v)) + torch.sqrt(2.0 * v / math.pi) * torch.exp(-d * d / (2.0 * v))


def mixture_crps_dense(raw: torch.Tensor, y, weights=None, outputs=CRPS_OUTPUTS, budget: int = 1 << 24) -> dict:
    """The exact CRPS of the predictive mixture in torch float64, on raw's device: raw [C, S, N, 2] (mu, log sigma), y [N],
    weights as ``crps_weights`` takes them -> the ``outputs`` asked for among ``crps_chain``, ``spread_chain`` [C, N],
    ``crps_mix``, ``spread_mix`` [1 + n_w, N] (row 0 the pooled ensemble, w_c = K_c / sum K), ``gram`` [N, C, C] and
    ``dropped`` [C, N] int32 -- what ``Engine.mixture_crps`` computes, with every pair term in fp64.  The pairs go in chunks of
    at most ``budget`` terms.  A draw with a non-finite output on a row is left out of that row; a chain with nothing kept has
    NaN in its own outputs, is skipped by the pooled weights and makes a weighted mixture that uses it NaN."""
    outputs = tuple(outputs)
    if not outputs or any(k not in CRPS_OUTPUTS for k in outputs):
        raise ValueError(f'outputs: a non-empty choice of {CRPS_OUTPUTS}')
    if raw.ndim != 4 or raw.shape[-1] != 2:
        raise ValueError('raw must be [C, S, N, 2]')
    C, S, N = (int(v) for v in raw.shape[:3])
    W = crps_weights(weights, C).to(raw.device)
    ok = torch.isfinite(raw).all(dim=-1)                                   # [C, S, N]
    o = torch.where(ok[..., None], raw, torch.zeros_like(raw)).to(torch.float64)
    mu, var = o[..., 0], torch.exp(o[..., 1]).clamp(min=1e-6, max=1e6) ** 2
    okf = ok.to(torch.float64)
    K = okf.sum(dim=1)                                                     # [C, N]
    yv = torch.as_tensor(y, device=raw.device).to(torch.float64).reshape(-1)
    if yv.shape != (N,):
        raise ValueError('y must be [N]')
    a = (_abs_normal_mean(yv[None, None] - mu, var) * okf).sum(dim=1) / K  # [C, N]
    G = torch.empty((N, C, C), dtype=torch.float64, device=raw.device)
    step = max(1, budget // max(1, S * N))
    for c in range(C):
        for c2 in range(c, C):
            tot = torch.zeros(N, dtype=torch.float64, device=raw.device)
            for i0 in range(0, S, step):
                d = mu[c, i0:i0 + step, None] - mu[c2, None]              # [i, S, N]
                v = var[c, i0:i0 + step, None] + var[c2, None]
                tot += (_abs_normal_mean(d, v) * okf[c, i0:i0 + step, None] * okf[c2, None]).sum(dim=(0, 1))
            G[:, c, c2] = G[:, c2, c] = tot / (K[c] * K[c2])
    diag = torch.diagonal(G, dim1=1, dim2=2).T                            # [C, N]
    Ktot = K.sum(dim=0)
    pooled = torch.where(Ktot > 0, K / Ktot, torch.full_like(K, float('nan'))).T      # [N, C]
    t1, t2 = [], []
    for m in range(1 + W.shape[0]):
        w = pooled if m == 0 else W[m - 1][None].expand(N, C)
        ww = w[:, :, None] * w[:, None, :]
        t1.append(torch.where(w == 0, torch.zeros_like(w), w * a.T).sum(dim=1))
        t2.append(torch.where(ww == 0, torch.zeros_like(ww), ww * G).sum(dim=(1, 2)))
    t1, t2 = torch.stack(t1), torch.stack(t2)
    res = {'crps_chain': a - 0.5 * diag, 'spread_chain': 0.5 * diag, 'crps_mix': t1 - 0.5 * t2, 'spread_mix': 0.5 * t2,
           'gram': G, 'dropped': (S - ok.sum(dim=1)).to(torch.int32)}
    return {k: res[k] for k in outputs}


def crps_summary(rows: dict, weights=None) -> dict:
    """Totals of the per-row CRPS arrays (``Engine.crps_stream`` / ``mixture_crps_dense``), on the host in fp64.  Means run over
    the rows with a finite value, standard errors are sd / sqrt(rows).  ``crps``, ``crps_se``, ``spread``, ``spread_se``: the
    pooled ensemble (row 0 of the mix arrays); ``mix_crps`` ... ``mix_spread_se``: lists over the caller's weight vectors;
    ``chain_crps`` ... ``chain_spread_se``: lists over the chains.  With ``weights`` [n_w, C] (those of the call) also
    ``mix_pooling_gain``, the mean over rows of sum_c w_c crps_chain[c] - crps_mix: what pooling the chains gains over scoring
    them one by one, >= 0 up to rounding.  With ``gram`` also ``energy_distance`` [C][C], the row mean of
    2 G_cc' - G_cc - G_c'c'.  Keys whose arrays are absent are left out."""
    import numpy as np
    a = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float64)
         for k, v in rows.items() if k in CRPS_OUTPUTS and k != 'dropped'}

    def mean_se(x):
        out = []
        for r in np.atleast_2d(x):
            f = r[np.isfinite(r)]
            m = float(f.mean()) if f.size else float('nan')
            se = float(f.std(ddof=1) / math.sqrt(f.size)) if f.size > 1 else float('nan')
            out.append((m, se))
        return out

    res = {}
    for key, name in (('crps_mix', 'crps'), ('spread_mix', 'spread')):
        if key in a:
            ms = mean_se(a[key])
            res[name], res[name + '_se'] = ms[0]
            res['mix_' + name], res['mix_' + name + '_se'] = [m for m, _ in ms[1:]], [s for _, s in ms[1:]]
            res['n_rows'] = int(a[key].shape[1])
            res['rows_nan'] = int((~np.isfinite(a[key][0])).sum())
    for key, name in (('crps_chain', 'chain_crps'), ('spread_chain', 'chain_spread')):
        if key in a:
            ms = mean_se(a[key])
            res[name], res[name + '_se'] = [m for m, _ in ms], [s for _, s in ms]
    if weights is not None and 'crps_chain' in a and 'crps_mix' in a:
        W = crps_weights(weights, a['crps_chain'].shape[0]).numpy()
        gains = []
        for m in range(W.shape[0]):
            use = W[m] != 0
            g = (W[m][use, None] * a['crps_chain'][use]).sum(axis=0) - a['crps_mix'][1 + m]
            gains.append(mean_se(g)[0][0])
        res['mix_pooling_gain'] = gains
    if 'gram' in a:
        G = a['gram']
        d = np.diagonal(G, axis1=1, axis2=2)
        with np.errstate(invalid='ignore'):
            D2 = 2.0 * G - d[:, :, None] - d[:, None, :]
            fin = np.isfinite(D2)
            cnt = fin.sum(axis=0)
            res['energy_distance'] = (np.where(fin, D2, 0.0).sum(axis=0) / np.where(cnt > 0, cnt, 1)).tolist()
    return res


# ---- input sensitivities of the ensemble's predictions: the torch restatement of mile_predict_sensitivities
# (Engine.predict_sensitivities) in fp64 from the closed-form chain of matrices.  The tests' yardstick, and the fallback where
# the library refuses.

SENS_OUTPUTS = ('mean', 'sd', 'pos', 'dropped', 'chain_ape', 'chain_abs', 'chain_kept')


def sensitivity_jacobians(spec: ModelSpec, theta: torch.Tensor, X: torch.Tensor):
    """theta [M, d] draws and X [N, F] -> (raw outputs [M, N, O], J [M, N, P, F]) in theta's dtype.  Jraw[o][f] = d r_o / d x_f =
    [W_0 diag phi'(z_0) W_1 ... diag phi'(z_{L-2}) W_{L-1}]_{f,o}, phi' expressed through the activation's output (relu' = 1 iff
    z > 0); regression reports J = Jraw, classification J[k][f] = pi_k (Jraw[k][f] - sum_j pi_j Jraw[j][f]), pi = softmax(r)."""
    leaves = {n: (o, s) for n, o, s in spec.leaves()}
    nl = len(spec.hidden_structure)
    act = {'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}[spec.activation]
    dact = {'relu': lambda h: (h > 0).to(h.dtype), 'tanh': lambda h: 1.0 - h * h, 'sigmoid': lambda h: h * (1.0 - h)}[spec.activation]
    X = X.to(theta.device, theta.dtype)
    Ws, hs = [], []
    h = X[None].expand(theta.shape[0], -1, -1)
    for li in range(nl):
        ko, ks = leaves[f'{spec.root}.layer{li}.kernel']
        bo, bs = leaves[f'{spec.root}.layer{li}.bias']
        W = theta[:, ko:ko + ks[0] * ks[1]].reshape(-1, *ks)
        h = torch.baddbmm(theta[:, bo:bo + bs[0]][:, None, :], h, W)
        if li < nl - 1:
            h = act(h)
            hs.append(h)
        Ws.append(W)
    raw = h
    g = Ws[-1].transpose(1, 2)[:, None].expand(-1, X.shape[0], -1, -1)          # [M, N, P, width]: d r_p / d a_{L-1}
    for li in range(nl - 2, -1, -1):
        g = torch.matmul(g * dact(hs[li])[:, :, None, :], Ws[li].transpose(1, 2)[:, None])
    if spec.task not in ('regr', 'regression'):
        pi = torch.softmax(raw, dim=-1)
        g = pi[..., None] * (g - (pi[..., None] * g).sum(dim=2, keepdim=True))
    return raw, g


def sensitivities_dense(spec: ModelSpec, samples: torch.Tensor, X: torch.Tensor, batch: int = 64) -> dict:
    """Input sensitivities of ``samples`` [C, S, d] (or [S, d]: one chain) on X [N, F] in torch fp64 on the samples' device, ``batch``
    draws at a time: the dict of ``Engine.predict_sensitivities``.  Per row and column (p, f) over the kept draws of all chains:
    ``mean``, ``sd`` (ddof 1; 0 for one kept draw) and ``pos``, the share with J > 0, fp32 [N, P, F]; ``dropped`` int32 [N]; per
    chain over its kept (draw, row) pairs ``chain_ape`` (mean J), ``chain_abs`` (mean |J|) fp64 [C, P, F] and ``chain_kept`` int64
    [C].  A (draw, row) pair is kept iff its raw outputs and all its P * F entries are finite; a row or a chain with nothing kept
    holds NaN."""
    if not isinstance(spec, ModelSpec):
        raise ValueError('input sensitivities need an FCN (token ids and image pixels are out of scope)')
    samples = torch.as_tensor(samples)
    if samples.ndim == 2:
        samples = samples[None]
    C, S, d = samples.shape
    th = samples.reshape(C * S, d).to(torch.float64)
    X = torch.as_tensor(X).to(th.device, torch.float64)
    N, F, P = X.shape[0], X.shape[1], int(spec.hidden_structure[-1])
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=th.device)
    k, mean, M2, pos = z(N), z(N, P, F), z(N, P, F), z(N, P, F)
    csum, cabs, ckept = z(C, P, F), z(C, P, F), torch.zeros(C, dtype=torch.int64, device=th.device)
    for c in range(C):
        for b0 in range(c * S, (c + 1) * S, batch):
            raw, J = sensitivity_jacobians(spec, th[b0:min(b0 + batch, (c + 1) * S)], X)
            ok = torch.isfinite(raw).all(dim=-1) & torch.isfinite(J).all(dim=-1).all(dim=-1)          # [b, N]
            w = ok.to(torch.float64)[..., None, None]
            J = torch.where(ok[..., None, None], J, torch.zeros_like(J))
            kb = ok.sum(dim=0).to(torch.float64)
            mb = (J * w).sum(dim=0) / kb.clamp(min=1)[:, None, None]
            db = (J - mb) * w
            M2b = (db * db).sum(dim=0)
            kt = k + kb
            delta = mb - mean
            mean = mean + delta * (kb / kt.clamp(min=1))[:, None, None]                      # Chan's merge of the batch
            M2 = M2 + M2b + delta * delta * (k * kb / kt.clamp(min=1))[:, None, None]
            k = kt
            pos = pos + ((J > 0).to(torch.float64) * w).sum(dim=0)
            csum[c] += (J * w).sum(dim=(0, 1))
            cabs[c] += (J.abs() * w).sum(dim=(0, 1))
            ckept[c] += ok.sum()
    nan = torch.full_like(mean, float('nan'))
    kk = k[:, None, None]
    some = (kk > 0).expand_as(mean)
    sd = torch.where(kk > 1, torch.sqrt(M2 / (kk - 1).clamp(min=1)), torch.zeros_like(M2))
    ck = ckept.to(torch.float64)[:, None, None]
    cnan = torch.full_like(csum, float('nan'))
    return {'mean': torch.where(some, mean, nan).to(torch.float32), 'sd': torch.where(some, sd, nan).to(torch.float32),
            'pos': torch.where(some, pos / kk.clamp(min=1), nan).to(torch.float32), 'dropped': (C * S - k).to(torch.int32),
            'chain_ape': torch.where(ck > 0, csum / ck.clamp(min=1), cnan), 'chain_abs': torch.where(ck > 0, cabs / ck.clamp(min=1), cnan),
            'chain_kept': ckept}


def sensitivity_summary(result: dict, feature_names=None) -> dict:
    """What the sensitivities say per head output p, on the host in fp64, from the dict of ``Engine.predict_sensitivities`` /
    ``sensitivities_dense``: ``ape`` [P][F], the ensemble's average partial effect (the mean of ``chain_ape`` over the chains);
    ``importance`` [P][F], the mean of ``chain_abs``; ``chain_sd`` [P][F], the sd (ddof 1, 0 for one chain) of ``chain_ape``
    across the chains -- whether the chains agree on what matters; ``decided`` [P][F], the share of rows whose sign is decided
    (``pos`` >= 0.95 or <= 0.05; rows with nothing kept do not count); ``ranking`` [P][F], the features by falling importance,
    as indices, and ``ranked_names`` where ``feature_names`` is given.  Chains with nothing kept are left out of the chain
    statistics."""
    import numpy as np
    a = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in result.items()}
    ape, imp = a['chain_ape'].astype(np.float64), a['chain_abs'].astype(np.float64)
    use = np.isfinite(ape).all(axis=(1, 2)) & np.isfinite(imp).all(axis=(1, 2))
    ape, imp = ape[use], imp[use]
    P, F = ape.shape[1], ape.shape[2]
    if feature_names is not None and len(feature_names) != F:
        raise ValueError(f'feature_names: {F} names expected')
    pos = a['pos'].astype(np.float32)                                   # compared in its own format: 19 / 20 in fp32 is 0.95 in fp32
    rows = np.isfinite(pos).all(axis=(1, 2))
    decided = ((pos[rows] >= np.float32(0.95)) | (pos[rows] <= np.float32(0.05))).mean(axis=0) if rows.any() else np.full((P, F), np.nan)
    nan = np.full((P, F), np.nan)
    importance = imp.mean(axis=0) if len(imp) else nan
    ranking = np.argsort(-np.nan_to_num(importance, nan=-np.inf), axis=1, kind='stable')
    res = {'ape': (ape.mean(axis=0) if len(ape) else nan).tolist(), 'importance': importance.tolist(),
           'chain_sd': (ape.std(axis=0, ddof=1) if len(ape) > 1 else np.zeros((P, F)) if len(ape) else nan).tolist(),
           'decided': decided.tolist(), 'ranking': ranking.tolist(), 'n_chains': int(use.sum()), 'n_rows': int(rows.sum())}
    if feature_names is not None:
        res['feature_names'] = [str(n) for n in feature_names]
        res['ranked_names'] = [[str(feature_names[i]) for i in r] for r in ranking]
    return res


# ---- partial dependence and ICE curves of the ensemble's predictions: the grid, the torch restatement of
# mile_predict_partial_dependence (Engine.predict_partial_dependence) in fp64 on substituted tables -- the tests' and the timing
# tool's yardstick, and the fallback on the CPU and where the library refuses -- and what the curves say.

PD_OUTPUTS = ('ice_mean', 'ice_sd', 'dropped', 'curves', 'pd_mean', 'pd_sd', 'chain_pd', 'chain_draws')


def pd_grid(x, features, G: int, kind: str = 'quantile', lo: float = 0.05, hi: float = 0.95) -> torch.Tensor:
    """The grid [Fs, G] fp32 of ``features`` from the columns of the table x [N, F] itself: ``kind='quantile'`` the quantiles
    (linear interpolation) at G equally spaced levels from ``lo`` to ``hi``, so that every grid value lies where the data do;
    ``kind='linspace'`` G equally spaced values from the ``lo`` to the ``hi`` quantile.  G = 1: the (lo + hi) / 2 quantile.
    Non-finite entries of a column are left out.  On x's device for a tensor, on the host otherwise."""
    import numpy as np
    if kind not in ('quantile', 'linspace'):
        raise ValueError("kind: 'quantile' or 'linspace'")
    if G < 1 or not 0.0 <= lo <= hi <= 1.0:
        raise ValueError('G >= 1 and 0 <= lo <= hi <= 1 are needed')
    device = x.device if isinstance(x, torch.Tensor) else 'cpu'
    a = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float64)
    if a.ndim != 2:
        raise ValueError('x must be [N, F]')
    levels = np.linspace(lo, hi, G) if G > 1 else np.array([0.5 * (lo + hi)])
    rows = []
    for f in features:
        if not 0 <= int(f) < a.shape[1]:
            raise ValueError(f'feature {f} out of range (0 .. {a.shape[1] - 1})')
        col = a[:, int(f)]
        col = col[np.isfinite(col)]
        if not len(col):
            raise ValueError(f'feature {f} has no finite value')
        if kind == 'quantile':
            rows.append(np.quantile(col, levels))
        else:
            a0, a1 = np.quantile(col, [lo, hi])
            rows.append(np.linspace(a0, a1, G) if G > 1 else np.quantile(col, levels))
    return torch.from_numpy(np.asarray(rows, dtype=np.float64).reshape(len(rows), G).astype(np.float32)).to(device)


def _fcn_raw(spec: ModelSpec, theta: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
    """theta [M, d], X [N, F] -> the raw outputs [M, N, O] of the FCN in theta's dtype."""
    leaves = {n: (o, s) for n, o, s in spec.leaves()}
    nl = len(spec.hidden_structure)
    act = {'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}[spec.activation]
    h = X.to(theta.device, theta.dtype)[None].expand(theta.shape[0], -1, -1)
    for li in range(nl):
        ko, ks = leaves[f'{spec.root}.layer{li}.kernel']
        bo, bs = leaves[f'{spec.root}.layer{li}.bias']
        h = torch.baddbmm(theta[:, bo:bo + bs[0]][:, None, :], h, theta[:, ko:ko + ks[0] * ks[1]].reshape(-1, *ks))
        if li < nl - 1:
            h = act(h)
    return h


def partial_dependence_dense(engine_or_forward, samples, x, features, grid, batch: int = 0) -> dict:
    """Partial dependence and ICE curves of ``samples`` [C, S, d] (or [S, d]: one chain) on x [N, F] as the composition a user
    writes today: for every feature and grid value a copy of the table with the column replaced, forwarded, and the head
    outputs [C * S, N, G, P] of a feature reduced in torch fp64 -- the dict of ``Engine.predict_partial_dependence``.  The forward
    is ``engine_or_forward.predict`` for an Engine (fp32, on the device), the fp64 torch FCN for a ``ModelSpec`` (any device: the
    fallback), or a callable (theta [M, d], X [N, F]) -> raw [M, N, O] with ``task`` 'regr' assumed unless it has a ``task``
    attribute.  ``batch`` draws are forwarded at a time (0: 256 for the fp64 torch FCN, all of them otherwise).  The drop rule is per (draw, row, feature): kept iff all G * P values
    are finite; note that substitution, unlike the library's update z_0 + (v - x_f) W_0[f], takes a non-finite x_f out of the row."""
    if isinstance(engine_or_forward, ModelSpec):
        spec = engine_or_forward
        task, dtype = spec.task, torch.float64
        forward = lambda th, X: _fcn_raw(spec, th, X)
    elif hasattr(engine_or_forward, 'predict'):
        task, dtype = engine_or_forward.spec.task, torch.float32
        forward = engine_or_forward.predict
    else:
        task, dtype = getattr(engine_or_forward, 'task', 'regr'), torch.float32
        forward = engine_or_forward
    samples = torch.as_tensor(samples)
    if samples.ndim == 2:
        samples = samples[None]
    if samples.ndim != 3:
        raise ValueError('samples must be [C, S, d] or [S, d]')
    C, S, d = samples.shape
    th = samples.reshape(C * S, d).to(dtype)
    x = torch.as_tensor(x).to(th.device, dtype)
    grid = torch.as_tensor(grid).to(th.device, torch.float32)
    feats = [int(f) for f in features]
    if x.ndim != 2 or grid.ndim != 2 or grid.shape[0] != len(feats) or len(set(feats)) != len(feats) or not feats:
        raise ValueError('x must be [N, F], grid [Fs, G] with one row per distinct feature')
    if min(feats) < 0 or max(feats) >= x.shape[1]:
        raise ValueError('a feature index is out of range')
    M, N, G = C * S, x.shape[0], grid.shape[1]
    batch = int(batch) if batch > 0 else 256 if isinstance(engine_or_forward, ModelSpec) else M
    regr = task in ('regr', 'regression')
    res = {k: [] for k in PD_OUTPUTS}
    nan = float('nan')
    for i, f in enumerate(feats):
        cols = []
        for g in range(G):
            xs = x.clone()
            xs[:, f] = grid[i, g].to(dtype)
            raw = torch.cat([forward(th[b0:b0 + batch], xs) for b0 in range(0, M, batch)]).to(torch.float64)
            cols.append(raw if regr else torch.softmax(raw, dim=-1))
        h = torch.stack(cols, dim=2)                                             # [M, N, G, P]
        ok = torch.isfinite(h).all(dim=-1).all(dim=-1)                           # [M, N]
        w = ok.to(torch.float64)[..., None, None]
        h = torch.where(ok[..., None, None], h, torch.zeros_like(h))
        k = ok.sum(dim=0).to(torch.float64)[:, None, None]                       # kept draws per row
        mean = h.sum(dim=0) / k.clamp(min=1)
        dd = (h - mean) * w
        sd = torch.where(k > 1, torch.sqrt((dd * dd).sum(dim=0) / (k - 1).clamp(min=1)), torch.zeros_like(mean))
        some = (k > 0).expand_as(mean)
        res['ice_mean'].append(torch.where(some, mean, torch.full_like(mean, nan)).to(torch.float32))
        res['ice_sd'].append(torch.where(some, sd, torch.full_like(sd, nan)).to(torch.float32))
        res['dropped'].append((M - ok.sum(dim=0)).to(torch.int32))
        kr = ok.sum(dim=1)                                                       # kept rows per draw
        m = h.sum(dim=1) / kr.to(torch.float64).clamp(min=1)[:, None, None]      # [M, G, P]: the fp64 row means
        have = kr > 0
        res['curves'].append(torch.where(have[:, None, None], m, torch.full_like(m, nan)).to(torch.float32))

        def band(mm):
            n = mm.shape[0]
            if n == 0:
                return torch.full_like(m[0], nan), torch.full_like(m[0], nan)
            return mm.mean(dim=0), (mm.std(dim=0, unbiased=True) if n > 1 else torch.zeros_like(m[0]))

        pm, ps = band(m[have])
        res['pd_mean'].append(pm)
        res['pd_sd'].append(ps)
        res['chain_pd'].append(torch.stack([band(m[c * S:(c + 1) * S][have[c * S:(c + 1) * S]])[0] for c in range(C)]))
        res['chain_draws'].append(have.reshape(C, S).sum(dim=1).to(torch.int64))
    stack_at = {'ice_mean': 1, 'ice_sd': 1, 'dropped': 1, 'curves': 1, 'pd_mean': 0, 'pd_sd': 0, 'chain_pd': 1, 'chain_draws': 1}
    return {k: torch.stack(v, dim=stack_at[k]) for k, v in res.items()}


def partial_dependence_summary(res: dict, grid) -> dict:
    """What the curves say per selected feature i and head column p, on the host in fp64, from the dict of
    ``Engine.predict_partial_dependence`` / ``partial_dependence_dense`` and the grid [Fs, G]; every entry [Fs][P]:
    ``importance``, the sd (ddof 1, 0 for G = 1) of ``pd_mean`` over the grid (Greenwell et al. 2018); ``span``, its max - min;
    ``slope``, its least-squares slope on the grid values (0 for a constant grid); ``band``, the mean over the grid of ``pd_sd``,
    the posterior's uncertainty about the curve; ``chain_sd``, the sd over the chains (ddof 1, 0 for one chain; chains without a
    curve left out) of ``chain_pd``, averaged over the grid, and ``chain_ratio`` = chain_sd / band -- chains that hold different
    functions show a ratio near or above 1; ``ice_heterogeneity``, the sd over the rows (ddof 1) of the ICE curves each centred at
    its own mean over the grid, averaged over the grid: 0 for an additive effect, > 0 where the effect of the feature depends on
    the other inputs, which first-order sensitivities cannot show.  Rows with nothing kept are left out."""
    import numpy as np
    a = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in res.items()}
    g = (grid.detach().cpu().numpy() if isinstance(grid, torch.Tensor) else np.asarray(grid)).astype(np.float64)
    pm, ps = a['pd_mean'].astype(np.float64), a['pd_sd'].astype(np.float64)
    Fs, G, P = pm.shape
    if g.shape != (Fs, G):
        raise ValueError(f'grid must be [{Fs}, {G}]')
    with np.errstate(all='ignore'):
        gc = g - g.mean(axis=1, keepdims=True)
        den = (gc * gc).sum(axis=1)[:, None]
        slope = np.where(den > 0, (gc[:, :, None] * (pm - pm.mean(axis=1, keepdims=True))).sum(axis=1) / np.where(den > 0, den, 1.0), 0.0)
        band = ps.mean(axis=1)
        out = {'importance': pm.std(axis=1, ddof=1) if G > 1 else np.zeros((Fs, P)), 'span': pm.max(axis=1) - pm.min(axis=1),
               'slope': slope, 'band': band}
        if 'chain_pd' in a:
            cp = a['chain_pd'].astype(np.float64)
            cp = cp[np.isfinite(cp).all(axis=(1, 2, 3))]
            csd = cp.std(axis=0, ddof=1).mean(axis=1) if len(cp) > 1 else np.zeros((Fs, P)) if len(cp) else np.full((Fs, P), np.nan)
            out['chain_sd'] = csd
            out['chain_ratio'] = np.where(band > 0, csd / np.where(band > 0, band, 1.0), np.nan)      # no band: no ratio
            out['n_chains'] = int(len(cp))
        if 'ice_mean' in a:
            ice = a['ice_mean'].astype(np.float64)
            het = np.full((Fs, P), np.nan)
            for i in range(Fs):
                rows = ice[:, i][np.isfinite(ice[:, i]).all(axis=(1, 2))]                     # [n, G, P]
                if len(rows) > 1:
                    het[i] = (rows - rows.mean(axis=1, keepdims=True)).std(axis=0, ddof=1).mean(axis=0)
                elif len(rows) == 1:
                    het[i] = 0.0
            out['ice_heterogeneity'] = het
    # JSON has no NaN or inf: an entry that is not finite (nothing kept, no band) is None
    clean = lambda v: [clean(e) for e in v] if isinstance(v, list) else (v if math.isfinite(v) else None)
    return {k: (clean(v.tolist()) if isinstance(v, np.ndarray) else v) for k, v in out.items()}
