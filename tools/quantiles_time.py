"""Predictive-quantile timing: Engine.predict_quantiles (mile_predict_quantiles: the forward in row tiles, packed and solved
on the device) against the two ways to the same intervals without it, on the same draws:

    sampled   evaluate.py's coverage path: Engine.predict, one Normal variate per (draw, row) from a seeded generator
              (metrics.sample_from_predictions), a sort per row and linear interpolation (metrics._quantiles_linear) --
              Monte-Carlo quantiles, [S, N, 2] raw outputs and [S, N] draws held whole
    torch     Engine.predict, then metrics.mixture_quantiles (fp64 bisection, 200 sweeps) in chunks of rows

    python tools/quantiles_time.py [--reps 3] [--shapes stock large] [--coverages 0.5 0.75 0.9 0.95]

Shapes: the stock airfoil run (12 000 draws x 301 rows) and 32 000 draws x 9 000 rows (2.3 GB of raw outputs), both on the
stock net 5 -> [16, 16, 2] with N(0, 0.3^2) draws.  Host clock around work that ends in a device synchronise, best of
`reps` after one warm-up call (the torch restatement: one call, no warm-up).  Peak device memory per path: torch's peak allocation over the calls plus what the library
allocated itself.  Sweeps per row: the solver's own count (mile_debug_quantile_sweeps).  One JSON line per shape.
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from mile_amd import ModelSpec
from mile_amd import metrics as M
from mile_amd.engine import Engine
from tools.moments_time import SHAPES, measured


def torch_quantiles(raw, levels, budget=1 << 30):
    """metrics.mixture_quantiles over chunks of rows: its [S, rows, Q] fp64 intermediates stay under ``budget`` bytes."""
    S, N = raw.shape[0], raw.shape[1]
    step = max(1, budget // (S * len(levels) * 8))
    return torch.cat([M.mixture_quantiles(raw[:, r0:r0 + step], levels) for r0 in range(0, N, step)])


def once(fn):
    """(result, seconds, peak bytes of torch's allocations) of ONE call of fn: the 200-sweep restatement is not repeated."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    live, t0 = torch.cuda.memory_allocated(), time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return res, time.perf_counter() - t0, int(torch.cuda.max_memory_allocated() - live)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', nargs='+', default=['stock', 'large'], choices=sorted(SHAPES))
    ap.add_argument('--coverages', type=float, nargs='+', default=[0.5, 0.75, 0.9, 0.95])
    ap.add_argument('--skip-others', action='store_true', help='time predict_quantiles only (for a profiler run)')
    args = ap.parse_args()
    dev = 'cuda:0'
    spec = ModelSpec(5, (16, 16, 2))
    levels = M.interval_levels(args.coverages)
    g = torch.Generator(device=dev).manual_seed(0)
    for name in args.shapes:
        S, N = SHAPES[name]
        theta = 0.3 * torch.randn((S, spec.n_params), generator=g, device=dev)
        X = torch.randn((N, 5), generator=g, device=dev)
        eng = Engine(spec, X[:64], torch.zeros(64, device=dev), device=dev)      # a fresh handle: its workspace starts empty
        t_new, m_new = measured(lambda: eng.predict_quantiles(theta, X, levels), args.reps)
        rows, total, most = eng.debug_quantile_sweeps()
        rec = {'shape': name, 'S': S, 'N': N, 'Q': int(levels.numel()), 'kernel': eng.grad_kernel, 'raw_bytes': S * N * 2 * 4,
               'workspace_bytes': eng.predict_quantiles_workspace(S, N), 'device_s': t_new, 'device_peak_bytes': m_new,
               'sweeps_per_row': total / max(rows, 1), 'sweeps_most': most}
        if not args.skip_others:
            gen = torch.Generator(device=dev).manual_seed(42)
            sampled = lambda: M._quantiles_linear(M.sample_from_predictions(eng.predict(theta, X), 'regr', gen), levels)
            t_fwd, _ = measured(lambda: eng.predict(theta, X), args.reps)
            t_smp, m_smp = measured(sampled, args.reps)
            b, t_tch, m_tch = once(lambda: torch_quantiles(eng.predict(theta, X), levels))
            a, c = eng.predict_quantiles(theta, X, levels).double(), sampled().T.double()
            sd = (b[:, -1] - b[:, 0]).clamp(min=1e-30)[:, None]                  # the widest interval: the rows' scale
            rec.update(predict_only_s=t_fwd, sampled_s=t_smp, sampled_peak_bytes=m_smp, torch_s=t_tch, torch_peak_bytes=m_tch,
                       speedup_vs_sampled=t_smp / t_new, speedup_vs_torch=t_tch / t_new,
                       max_diff_vs_torch_over_width=float(((a - b).abs() / sd).max()),
                       max_sampling_error_over_width=float(((c - b).abs() / sd).max()))
        print(json.dumps(rec), flush=True)
        del eng, theta, X


if __name__ == '__main__':
    main()
