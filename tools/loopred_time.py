"""LOO-prediction timing: Engine.loo_predict_stream (mile_loo_predict_stream: one forward per (draw, row) in row tiles, the
PSIS weights and the weighted sums on the device, never a per-draw tensor at once) against the way to the same numbers
without it, Engine.pointwise_loglik + Engine.predict + metrics.loo_predict_columns + metrics.psis_expect_dense (two forwards
and the vectorised fp64 torch form on dense tensors), and against Engine.loo_stream on the same inputs, which does strictly
less work (no weights kept, no sums), on the same draws and the same device:

    python tools/loopred_time.py [--reps 2] [--shapes stock b2]

Shapes: the stock airfoil run (net 5 -> [16, 16, 2], 12 000 draws, 1052 train rows: the row in LDS) and the B2 schedule (net
5 -> [64, 64, 64, 2], 128 chains x 1000 kept draws, 1052 rows: S > 16 384, the row streamed from the packed copy), N(0, 0.1^2)
draws around 0.  Host clock around work that ends in a device synchronise; the paths alternate, `reps` runs each after one
warm-up call of the streamed path, the best and all runs reported.  Peak device memory per path: torch's peak allocation above
what was live before (the inputs), plus what the library allocated itself.  The streamed call's peak must stay within
loo_predict_stream_workspace + its outputs + the inputs: asserted.  One process, one JSON line per shape; about 30 s in all.
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
from tools.loo_time import SHAPES, once

KEYS = ('expect', 'posterior', 'ess_w', 'khat', 'elpd_loo')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--shapes', nargs='+', default=['stock', 'b2'], choices=sorted(SHAPES))
    ap.add_argument('--skip-dense', action='store_true', help='time the streamed calls only (for a profiler run)')
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
        stream = lambda: eng.loo_predict_stream(theta, X, y)
        loo = lambda: eng.loo_stream(theta, X, y)
        dense = lambda: M.psis_expect_dense(eng.pointwise_loglik(theta, X, y), M.loo_predict_columns(eng.predict(theta, X), y, 'regr'))
        ws = eng.loo_predict_stream_workspace(S, N)
        outputs = N * (2 * 4 * 8 + 3 * 8 + 4)
        inputs = theta.numel() * 4 + X.numel() * 4 + y.numel() * 4
        a, _, first_peak = once(stream)                                         # the warm-up call grows the workspace: its peak is the call's
        t_new, t_loo, t_old, m_new, m_old, b = [], [], [], [first_peak], [], None
        for _ in range(args.reps):                                              # alternating
            a, t, m = once(stream)
            t_new.append(t)
            m_new.append(m)
            _, t, _ = once(loo)
            t_loo.append(t)
            if not args.skip_dense:
                b, t, m = once(dense)
                t_old.append(t)
                m_old.append(m)
        rec = {'shape': name, 'net': [5, *hs], 'S': S, 'N': N, 'kernel': eng.grad_kernel, 'workspace_bytes': ws,
               'stream_s': min(t_new), 'stream_runs_s': t_new, 'stream_peak_bytes': max(m_new),
               'stream_peak_allowed_bytes': ws + outputs + inputs, 'loo_stream_s': min(t_loo), 'ratio_to_loo_stream': min(t_new) / min(t_loo),
               'khat_above_0.7_share': float((a['khat'] > 0.7).double().mean()), 'ess_w_min': float(a['ess_w'].min())}
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
