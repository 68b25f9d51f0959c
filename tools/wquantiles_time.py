"""Chain-weighted predictive-quantile timing: Engine.predict_quantiles_weighted (mile_predict_quantiles_weighted) against
Engine.predict_quantiles (mile_predict_quantiles, whose kernels this feature leaves as they were) on the same draws, and
against the torch fp64 form (Engine.predict, then metrics.weighted_mixture_quantiles: 200 bisection sweeps, rows in chunks):

    python tools/wquantiles_time.py [--reps 3] [--shapes stock large] [--chains 12] [--coverages 0.5 0.75 0.9 0.95]

Shapes: those of tools/quantiles_time.py (the stock airfoil run, 12 000 draws x 301 rows, and 32 000 draws x 9 000 rows) on
the stock net 5 -> [16, 16, 2] with N(0, 0.3^2) draws, split as ``--chains`` chains (the draws that do not fill a chain are
left out) with Dirichlet weights.  Host clock around
work that ends in a device synchronise, best of ``reps`` after one warm-up call (the torch form: one call).  ``ratio`` is
weighted over unweighted: the weighted sweep adds a table lookup and a multiply per component and a counting prologue per
row, and takes its bracket in the solve kernel instead of the pack kernel.  One JSON line per shape.

Measured on an MI355X, 12 chains x 1 000 draws x 301 rows, Q = 8: weighted 3.71 ms, unweighted 3.09 ms, ratio 1.20 (1.24 with
the forward's 0.50 ms taken off both), torch fp64 944 ms (255x), device - torch 2.8e-8 of the widest interval (DESIGN.md
section 3.2o); 12 x 2 666 x 9 000: 201.7 ms against 189.9 ms, ratio 1.06.
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from mile_amd import ModelSpec
from mile_amd import metrics as M
from mile_amd.engine import Engine
from tools.moments_time import SHAPES, measured
from tools.quantiles_time import once


def torch_weighted_quantiles(raw, w, levels, budget=1 << 30):
    """metrics.weighted_mixture_quantiles over chunks of rows: its [C * S, rows, Q] fp64 intermediates stay under ``budget``."""
    D, N = raw.shape[0] * raw.shape[1], raw.shape[2]
    step = max(1, budget // (D * len(levels) * 8))
    return torch.cat([M.weighted_mixture_quantiles(raw[:, :, r0:r0 + step], w, levels) for r0 in range(0, N, step)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', nargs='+', default=['stock', 'large'], choices=sorted(SHAPES))
    ap.add_argument('--chains', type=int, default=12)
    ap.add_argument('--coverages', type=float, nargs='+', default=[0.5, 0.75, 0.9, 0.95])
    ap.add_argument('--skip-torch', action='store_true', help='time the two device paths only')
    args = ap.parse_args()
    dev = 'cuda:0'
    spec = ModelSpec(5, (16, 16, 2))
    levels = M.interval_levels(args.coverages)
    g = torch.Generator(device=dev).manual_seed(0)
    torch.manual_seed(0)
    w = torch.distributions.Dirichlet(torch.ones(args.chains, dtype=torch.float64)).sample()
    w = w / w.sum()
    for name in args.shapes:
        D, N = SHAPES[name]
        D -= D % args.chains                                                     # whole chains: 32 000 draws are 12 x 2 666
        theta = 0.3 * torch.randn((args.chains, D // args.chains, spec.n_params), generator=g, device=dev)
        X = torch.randn((N, 5), generator=g, device=dev)
        eng = Engine(spec, X[:64], torch.zeros(64, device=dev), device=dev)      # a fresh handle: its workspace starts empty
        t_w, m_w = measured(lambda: eng.predict_quantiles_weighted(theta, X, w, levels), args.reps)
        t_u, m_u = measured(lambda: eng.predict_quantiles(theta, X, levels), args.reps)
        t_fwd, _ = measured(lambda: eng.predict(theta, X), args.reps)
        rec = {'shape': name, 'C': args.chains, 'S': D // args.chains, 'N': N, 'Q': int(levels.numel()), 'kernel': eng.grad_kernel,
               'weighted_s': t_w, 'unweighted_s': t_u, 'ratio': t_w / t_u, 'predict_only_s': t_fwd,
               'ratio_without_forward': (t_w - t_fwd) / max(t_u - t_fwd, 1e-12), 'weighted_peak_bytes': m_w, 'unweighted_peak_bytes': m_u,
               'workspace_bytes': eng.predict_quantiles_weighted_workspace(args.chains, D // args.chains, N)}
        if not args.skip_torch:
            b, t_tch, m_tch = once(lambda: torch_weighted_quantiles(eng.predict(theta, X), w, levels))
            a = eng.predict_quantiles_weighted(theta, X, w, levels).double()
            width = (b[:, -1] - b[:, 0]).clamp(min=1e-30)[:, None]               # the widest interval: the rows' scale
            rec.update(torch_s=t_tch, torch_peak_bytes=m_tch, speedup_vs_torch=t_tch / t_w,
                       max_diff_vs_torch_over_width=float(((a - b).abs() / width).max()))
        print(json.dumps(rec), flush=True)
        del eng, theta, X


if __name__ == '__main__':
    main()
