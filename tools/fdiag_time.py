"""Function-space chain diagnostics timing: Engine.function_diagnostics (mile_function_diagnostics: rows in tiles, the columns
packed on the device straight into the layout the diagnostic kernels read) against the dense composition -- Engine.predict
followed by metrics.function_diagnostics_dense, which holds predict's [C, S, N, O] tensor, the columns [C, S, M] and the
library's transposed copy at once.

    python tools/fdiag_time.py [--reps 3] [--shapes stock classification] [--rows-per-tile K]

Shapes: the stock airfoil run (12 chains x 1000 draws of the net 5 -> [16, 16, 2], the 301 rows of its test split's size) and
a classification net 8 -> [32, 32, 7] sigmoid with 8 chains x 500 draws on 200 rows; N(0, 0.3^2) draws, normal rows.  Host
clock around work that ends in a device synchronise, best of `reps` after one warm-up call.  Peak device memory per path:
torch.cuda.max_memory_allocated above what was live before, plus what the library allocated itself (the drop in free device
memory that torch's own reservations do not explain).  One JSON line per shape.
"""
import argparse
import json
import sys
import time
import warnings
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from mile_amd import ModelSpec
from mile_amd import metrics as M
from mile_amd.engine import Engine

#          F  hidden_structure  activation  task              C   S     N
SHAPES = {'stock': (5, (16, 16, 2), 'relu', 'regr', 12, 1000, 301),
          'classification': (8, (32, 32, 7), 'sigmoid', 'classification', 8, 500, 200)}


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
    ap.add_argument('--shapes', nargs='+', default=['stock', 'classification'], choices=sorted(SHAPES))
    ap.add_argument('--rows-per-tile', type=int, default=0)
    ap.add_argument('--skip-dense', action='store_true', help='time the library call only (for a profiler run)')
    args = ap.parse_args()
    dev = 'cuda:0'
    warnings.simplefilter('ignore', UserWarning)
    g = torch.Generator(device=dev).manual_seed(0)
    for name in args.shapes:
        F_, hs, act, task, C_, S, N = SHAPES[name]
        spec = ModelSpec(F_, hs, activation=act, task=task)
        theta = 0.3 * torch.randn((C_, S, spec.n_params), generator=g, device=dev)
        X = torch.randn((N, F_), generator=g, device=dev)
        y = torch.randn(N, generator=g, device=dev) if task == 'regr' else torch.randint(0, hs[-1], (N,), generator=g, device=dev)
        eng = Engine(spec, X[:64], y[:64], device=dev)                       # a fresh handle: its workspace starts empty
        fused = lambda: eng.function_diagnostics(theta, X, y, max_rows_per_tile=args.rows_per_tile)
        t_new, m_new = measured(fused, args.reps)
        Q = hs[-1] + 1
        rec = {'shape': name, 'C': C_, 'S': S, 'N': N, 'M': N * Q + 1, 'kernel': eng.grad_kernel, 'rows_per_tile': args.rows_per_tile,
               'workspace_bytes': eng.function_diagnostics_workspace(C_, S, N), 'fused_s': t_new, 'fused_peak_bytes': m_new}
        if not args.skip_dense:
            dense = lambda: M.function_diagnostics_dense(eng.predict(theta, X), y, task, 2)
            t_old, m_old = measured(dense, args.reps)
            a, b = fused(), dense()
            rec.update(dense_s=t_old, dense_peak_bytes=m_old, speedup=t_old / t_new,
                       max_rel_diff={k: float(((a[k] - b[k]).abs() / b[k].abs().clamp(min=1e-30)).max())
                                     for k in ('wcv', 'bcv', 'ess', 'crhat', 'rhat')})
        print(json.dumps(rec), flush=True)
        del eng, theta, X, y


if __name__ == '__main__':
    main()
