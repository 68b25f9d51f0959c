"""PSIS-LOO timing: Engine.loo_stream (mile_loo_stream: the forward in row tiles, packed and reduced per row on the device,
never [S, N] at once) against the way to the same numbers without it, Engine.pointwise_loglik + metrics.psis_loo (the
vectorised fp64 torch restatement) on the dense tensor, on the same draws and the same device:

    python tools/loo_time.py [--reps 3] [--shapes stock b2]

Shapes: the stock airfoil run (net 5 -> [16, 16, 2], 12 000 draws, 1052 train rows) and the B2 schedule (net
5 -> [64, 64, 64, 2], 128 chains x 1000 kept draws, 1052 rows: 539 MB of pointwise log-likelihoods), N(0, 0.1^2) draws around
0.  Host clock around work that ends in a device synchronise; the two paths alternate, `reps` runs each after one warm-up
call of the streamed path, the best and all runs reported.  Peak device memory per path: torch's peak allocation above what
was live before (the inputs), plus what the library allocated itself.  The streamed call's peak must stay within
loo_stream_workspace + its outputs + the inputs (the handle's staged copy of the rows): asserted.  One JSON line per shape.
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

SHAPES = {'stock': ((16, 16, 2), 12000, 1052), 'b2': ((64, 64, 64, 2), 128000, 1052)}
KEYS = ('lppd', 'p_waic', 'elpd_loo', 'khat')


def once(fn):
    """(result, seconds, peak bytes) of one call of fn: torch's peak above what was live, plus the library's own allocations."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    live, free0, res0 = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    lib = (free0 - torch.cuda.mem_get_info()[0]) - (torch.cuda.memory_reserved() - res0)
    return res, dt, int(torch.cuda.max_memory_allocated() - live + max(lib, 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', nargs='+', default=['stock', 'b2'], choices=sorted(SHAPES))
    ap.add_argument('--skip-dense', action='store_true', help='time loo_stream only (for a profiler run)')
    args = ap.parse_args()
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    for name in args.shapes:
        hs, S, N = SHAPES[name]
        spec = ModelSpec(5, hs)
        theta = 0.1 * torch.randn((S, spec.n_params), generator=g, device=dev)
        X = torch.randn((N, 5), generator=g, device=dev)
        y = torch.randn(N, generator=g, device=dev)
        eng = Engine(spec, X[:64], y[:64], device=dev)                          # a fresh handle: its workspace starts empty
        stream = lambda: eng.loo_stream(theta, X, y)
        dense = lambda: M.psis_loo(eng.pointwise_loglik(theta, X, y))
        ws = eng.loo_stream_workspace(S, N)
        outputs = N * (4 * 8 + 4)
        inputs = theta.numel() * 4 + X.numel() * 4 + y.numel() * 4
        a, _, first_peak = once(stream)                                         # the warm-up call grows the workspace: its peak is the call's
        t_new, t_old, m_new, m_old, b = [], [], [first_peak], [], None
        for _ in range(args.reps):                                              # alternating
            a, t, m = once(stream)
            t_new.append(t)
            m_new.append(m)
            if not args.skip_dense:
                b, t, m = once(dense)
                t_old.append(t)
                m_old.append(m)
        rec = {'shape': name, 'net': [5, *hs], 'S': S, 'N': N, 'kernel': eng.grad_kernel, 'pointwise_bytes': S * N * 4,
               'workspace_bytes': ws, 'stream_s': min(t_new), 'stream_runs_s': t_new, 'stream_peak_bytes': max(m_new),
               'stream_peak_allowed_bytes': ws + outputs + inputs,
               'n_khat_above_0.7': int((a['khat'] > 0.7).sum()), 'n_khat_nofit': int(torch.isnan(a['khat']).sum())}
        assert rec['stream_peak_bytes'] <= rec['stream_peak_allowed_bytes'], rec
        if b is not None:
            rec.update(dense_s=min(t_old), dense_runs_s=t_old, dense_peak_bytes=max(m_old), speedup=min(t_old) / min(t_new))
            for k in KEYS:
                fin = ~torch.isnan(b[k])
                assert bool((torch.isnan(a[k]) == torch.isnan(b[k])).all()), k
                rec[f'max_diff_{k}'] = float(((a[k] - b[k])[fin].abs() / b[k][fin].abs().clamp(min=1.0)).max()) if bool(fin.any()) else 0.0
        print(json.dumps(rec), flush=True)
        del eng, theta, X, y, a, b


if __name__ == '__main__':
    main()
