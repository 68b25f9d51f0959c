"""Posterior-predictive moments timing: Engine.predict_moments (mile_predict_moments: the forward in passes, reduced on the
device) against Engine.predict followed by metrics.predictive_moments on the same draws (raw outputs [S, N, O] held whole).

    python tools/moments_time.py [--reps 3] [--shapes stock large] [--draws-per-pass K]

Shapes: the stock airfoil run (12 000 draws x 301 rows) and 32 000 draws x 9 000 rows (2.3 GB of raw outputs: the largest
of the two where the unfused path still fits comfortably), both on the stock net 5 -> [16, 16, 2] with N(0, 0.3^2) draws.
Host clock around work that ends in a device synchronise, best of `reps` after one warm-up call.  Peak device memory per
path: torch's peak allocation over the calls plus what the library allocated itself (the drop in free device memory that
torch's own reservations do not explain).  One JSON line per shape.
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

SHAPES = {'stock': (12000, 301), 'large': (32000, 9000)}


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


def measured(fn, reps):
    """(best seconds, peak bytes) of fn: torch's peak allocation above what was live before, plus the library's own."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    live, free0, res0 = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
    t = best(fn, reps)
    lib = (free0 - torch.cuda.mem_get_info()[0]) - (torch.cuda.memory_reserved() - res0)
    return t, int(torch.cuda.max_memory_allocated() - live + max(lib, 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', nargs='+', default=['stock', 'large'], choices=sorted(SHAPES))
    ap.add_argument('--draws-per-pass', type=int, default=0)
    ap.add_argument('--skip-unfused', action='store_true', help='time predict_moments only (for a profiler run)')
    args = ap.parse_args()
    dev = 'cuda:0'
    spec = ModelSpec(5, (16, 16, 2))
    g = torch.Generator(device=dev).manual_seed(0)
    for name in args.shapes:
        S, N = SHAPES[name]
        theta = 0.3 * torch.randn((S, spec.n_params), generator=g, device=dev)
        X = torch.randn((N, 5), generator=g, device=dev)
        eng = Engine(spec, X[:64], torch.zeros(64, device=dev), device=dev)      # a fresh handle: its workspace starts empty
        t_new, m_new = measured(lambda: eng.predict_moments(theta, X, max_draws_per_pass=args.draws_per_pass), args.reps)
        rec = {'shape': name, 'S': S, 'N': N, 'kernel': eng.grad_kernel, 'draws_per_pass': args.draws_per_pass,
               'raw_bytes': S * N * 2 * 4, 'fused_s': t_new, 'fused_peak_bytes': m_new}
        if not args.skip_unfused:
            t_fwd, _ = measured(lambda: eng.predict(theta, X), args.reps)
            t_old, m_old = measured(lambda: M.predictive_moments(eng.predict(theta, X), 'regr'), args.reps)
            a, b = eng.predict_moments(theta, X), M.predictive_moments(eng.predict(theta, X), 'regr')
            rec.update(predict_only_s=t_fwd, unfused_s=t_old, unfused_peak_bytes=m_old, speedup=t_old / t_new,
                       max_rel_diff=[float(v) for v in ((a - b).abs() / b.abs().clamp(min=1e-30)).max(dim=0).values])
        print(json.dumps(rec), flush=True)
        del eng, theta, X


if __name__ == '__main__':
    main()
