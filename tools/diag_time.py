"""Chain-diagnostics timing: mile_amd.metrics.chain_diagnostics (mile_chain_diagnostics, all five statistics of ALL d
parameters) against the path evaluate.py had before it: metrics.effective_sample_size (ESS only) on a 256-column subset.

    python tools/diag_time.py [--reps 3] [--shapes stock b2]

Shapes: [12, 1000, 530] (stock net) and [128, 1000, 8834] (B2), synthetic AR(1) draws generated on the device (phi ~
U(-0.5, 0.98) per column, chain offsets 0.3 N(0,1)).  Host clock around work that ends in a device synchronise, best of
`reps` after one warm-up call.  One JSON line per shape: seconds per call and microseconds per column for both paths.
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from mile_amd import metrics as M

SHAPES = {'stock': (12, 1000, 530), 'b2': (128, 1000, 8834)}


def ar1(C, S, d, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    phi = torch.rand(d, generator=g, device=dev) * 1.48 - 0.5
    x = torch.empty((C, S, d), device=dev)
    x[:, 0] = torch.randn((C, d), generator=g, device=dev) / torch.sqrt(1 - phi ** 2)
    for t in range(1, S):
        x[:, t] = phi * x[:, t - 1] + torch.randn((C, d), generator=g, device=dev)
    return x + 0.3 * torch.randn((C, 1, d), generator=g, device=dev)


def best(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', nargs='+', default=['stock', 'b2'], choices=sorted(SHAPES))
    ap.add_argument('--old-cols', type=int, default=256, help='columns of the old path (evaluate.py --ess-params)')
    ap.add_argument('--skip-old', action='store_true', help='time the new path only (for a profiler run)')
    args = ap.parse_args()
    dev = 'cuda:0'
    for name in args.shapes:
        C, S, d = SHAPES[name]
        x = ar1(C, S, d, 1, dev)
        cols = np.sort(np.random.default_rng(0).choice(d, size=min(args.old_cols, d), replace=False))
        sub = x[:, :, torch.from_numpy(cols).to(dev)].contiguous()
        t_new = best(lambda: M.chain_diagnostics(x, 2), args.reps)
        rec = {'shape': name, 'C': C, 'S': S, 'd': d, 'path': M.LAST_DIAG_PATH, 'new_s': t_new, 'new_us_per_col': 1e6 * t_new / d}
        if not args.skip_old:
            t_old = best(lambda: M.effective_sample_size(sub), max(1, args.reps - 1))
            new = M.chain_diagnostics(sub, 2)['ess']
            old = M.effective_sample_size(sub)
            rec.update(old_cols=int(len(cols)), old_s=t_old, old_us_per_col=1e6 * t_old / len(cols),
                       per_col_speedup=(t_old / len(cols)) / (t_new / d),
                       ess_median_rel_diff=float(((new - old).abs() / old.abs()).median()))
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
