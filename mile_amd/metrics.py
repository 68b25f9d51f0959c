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
