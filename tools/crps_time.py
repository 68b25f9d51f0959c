"""CRPS timing: Engine.crps_stream (mile_crps_stream: the forward in row tiles, then all pairs of draws in k_crps_pairs) against
Engine.predict + metrics.mixture_crps_dense (the torch fp64 form, chunked over pairs) on the same draws and the same device:

    python tools/crps_time.py [--reps 3] [--shapes stock b2] [--dense-rows 0]

Shapes [C, S, N]: the stock airfoil run (12 chains x 1000 draws, 301 test rows) and the B2 schedule (128 x 1000, 301 rows), on
the stock net 5 -> 16 -> 16 -> 2 with synthetic rows and draws; ``tiny`` is for the tests.  The dense form costs two fp64
transcendentals per pair: with ``--dense-rows R`` it runs on the first R rows only (0: all rows, but 2 at B2) and ``dense_s`` is
that time scaled to all rows (``dense_rows`` says how many were run).  Host clock around work that ends in a device
synchronise; `reps` runs of each after one warm-up, the best and all runs reported.  ``pairs``: C S (C S + 1) / 2 per row, what the kernel evaluates.
``pair_kernel``: Engine.mixture_crps on predict's outputs held whole -- pack, pairs and finish without the forward -- whose rate
``pairs_per_s`` stands against ``valu_bound_pairs_per_s`` = CUs x 4 SIMDs x 32 lanes x clock / ``--valu-per-pair`` (the VALU
instructions of k_crps_pairs' inner loop per pair term, counted from the kernel's ISA; v_rsq_f32 and v_exp_f32 issue at half
rate and are counted twice).  ``launch_s_at_limit``: the time of one pair launch at CRPS_MAX_PAIRS_PER_LAUNCH at that rate.
Peak device memory per path: torch's peak allocation above what was live before, plus the library's workspace.  One JSON line
per shape.
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

SHAPES = {'stock': (12, 1000, 301), 'b2': (128, 1000, 301), 'tiny': (3, 40, 17)}
OUT = ('crps_chain', 'spread_chain', 'crps_mix', 'spread_mix', 'dropped')
MAX_PAIRS_PER_LAUNCH = 1 << 37          # CRPS_MAX_PAIRS_PER_LAUNCH (mile_crps.h)


def once(fn):
    """(result, seconds, peak bytes) of one call of fn: torch's peak allocation above what was live before."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return res, dt, int(torch.cuda.max_memory_allocated() - live)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', nargs='+', default=['stock', 'b2'], choices=sorted(SHAPES))
    ap.add_argument('--dense-rows', type=int, default=0, help='rows the dense form runs on (0: all, but 2 at the b2 shape)')
    ap.add_argument('--skip-dense', action='store_true', help='time the kernels only (for a profiler run)')
    ap.add_argument('--valu-per-pair', type=float, default=0.0, help='VALU issue slots per pair term of the inner loop (0: no bound reported)')
    ap.add_argument('--clock-mhz', type=float, default=2400.0, help='engine clock behind the VALU bound (MI355X: 2400 peak)')
    args = ap.parse_args()
    dev = 'cuda:0'
    g = torch.Generator().manual_seed(0)
    spec = ModelSpec(5, (16, 16, 2))
    eng = Engine(spec, torch.randn((64, 5), generator=g), torch.randn(64, generator=g), device=dev)
    props = torch.cuda.get_device_properties(0)
    for name in args.shapes:
        C_, S_, N = SHAPES[name]
        samples = (0.3 * torch.randn((C_, S_, eng.d), generator=g)).to(dev)
        X = torch.randn((N, 5), generator=g).to(dev)
        y = torch.randn(N, generator=g).to(dev)
        w = torch.full((1, C_), 1.0 / C_, dtype=torch.float64)
        D = C_ * S_
        pairs = D * (D + 1) // 2 * N
        rows = min(N, args.dense_rows) if args.dense_rows > 0 else (2 if name == 'b2' else N)
        stream = lambda: eng.crps_stream(samples, X, y, weights=w, outputs=OUT)
        raw = eng.predict(samples, X)
        kernel = lambda: eng.mixture_crps(raw, y, weights=w, outputs=OUT)
        dense = lambda: M.mixture_crps_dense(eng.predict(samples, X[:rows]), y[:rows], w, outputs=OUT)
        once(stream)
        t_new, m_new, t_k, t_old, m_old, a, b = [], [], [], [], [], None, None
        for _ in range(args.reps):
            a, t, m = once(stream)
            t_new.append(t)
            m_new.append(m)
            t_k.append(once(kernel)[1])
        ws = eng.crps_stream_workspace(C_, S_, N)
        rate = pairs / min(t_k)
        rec = {'shape': name, 'C': C_, 'S': S_, 'N': N, 'pairs': pairs, 'stream_s': min(t_new), 'stream_runs_s': t_new,
               'stream_peak_bytes': max(m_new) + ws, 'stream_workspace_bytes': ws, 'pair_kernel_s': min(t_k), 'pair_kernel_runs_s': t_k,
               'pairs_per_s': rate, 'launch_s_at_limit': MAX_PAIRS_PER_LAUNCH / rate, 'raw_bytes': raw.numel() * 4}
        if args.valu_per_pair > 0:
            bound = props.multi_processor_count * 128 * args.clock_mhz * 1e6 / args.valu_per_pair
            rec.update(valu_per_pair=args.valu_per_pair, valu_bound_pairs_per_s=bound, of_valu_bound=rate / bound)
        if not args.skip_dense:
            once(dense)
            for _ in range(args.reps if rows == N else 1):
                b, t, m = once(dense)
                t_old.append(t * N / rows)
                m_old.append(m)
            rec.update(dense_rows=rows, dense_s=min(t_old), dense_runs_s=t_old, dense_peak_bytes=max(m_old), speedup=min(t_old) / min(t_new))
            for k in ('crps_chain', 'crps_mix', 'spread_mix'):
                rec[f'max_rel_diff_{k}'] = float(((a[k][:, :rows] - b[k]).abs() / b[k].abs().clamp(min=1e-300)).max())
        print(json.dumps(rec), flush=True)
        del samples, raw, a, b


if __name__ == '__main__':
    main()
