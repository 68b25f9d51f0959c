"""Calibration timing: Engine.calibration_stream (mile_calibration_stream: the forward in row tiles and draw passes, folded into
per-chain fp64 sums on the device, never [C, S, N, K] at once) against the way to the same numbers without it,
Engine.predict in chunks into one [C, S, N, K] tensor + metrics.classification_calibration (the fp64 torch form), on the
same draws and the same device:

    python tools/calib_time.py [--reps 3] [--shapes covertype binary] [--rows N]

Shapes: covertype-like (54 features, net [64, 64, 7], 12 chains x 1000 draws) and a binary one (14 features, net [32, 32, 2],
12 x 1000), N(0, 0.3^2) draws around 0, on `--rows` rows (default 20 000: 6.7 GB of logits at K = 7, about as much as the
torch form's fp64 temporaries leave room for beside it).  Host clock around work that ends in a device synchronise; the two
paths alternate, `reps` runs each after one warm-up call of the streamed path, the best and all runs reported.  Also timed:
Engine.calibration on the held tensor (the calibration kernels alone, no forward) and Engine.predict alone (the forward
alone).  Peak device memory per path: torch's peak allocation above what was live before (the inputs), plus what the library
allocated itself.  The streamed call's peak must stay within calibration_stream_workspace + its outputs + the inputs (the
handle's staged copy of the rows): asserted.  One JSON line per shape.
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

SHAPES = {'covertype': (54, (64, 64, 7), 12, 1000), 'binary': (14, (32, 32, 2), 12, 1000)}
COVERAGES = (0.5, 0.75, 0.9, 0.95)
N_BINS = 15


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
    ap.add_argument('--shapes', nargs='+', default=['covertype', 'binary'], choices=sorted(SHAPES))
    ap.add_argument('--rows', type=int, default=20000)
    ap.add_argument('--draws', type=int, default=None, help='draws per chain (default: the shape\'s 1000)')
    ap.add_argument('--skip-dense', action='store_true', help='time calibration_stream only (for a profiler run)')
    args = ap.parse_args()
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    for name in args.shapes:
        F, hs, C_, S_ = SHAPES[name]
        S_ = args.draws or S_
        N, K = args.rows, hs[-1]
        spec = ModelSpec(F, hs, activation='relu', task='classification')
        theta = 0.3 * torch.randn((C_, S_, spec.n_params), generator=g, device=dev)
        X = torch.randn((N, F), generator=g, device=dev)
        y = torch.randint(0, K, (N,), generator=g, device=dev, dtype=torch.int32)
        eng = Engine(spec, X[:64], y[:64], device=dev)                          # a fresh handle: its workspace starts empty

        def predict_all():
            raw = torch.empty((C_, S_, N, K), dtype=torch.float32, device=dev)
            for c in range(C_):
                for s0 in range(0, S_, 100):
                    raw[c, s0:s0 + 100] = eng.predict(theta[c, s0:s0 + 100], X)
            return raw
        stream = lambda: eng.calibration_stream(theta, X, y, COVERAGES, N_BINS)
        dense = lambda: M.classification_calibration(predict_all(), y, COVERAGES, N_BINS)
        ws = eng.calibration_stream_workspace(C_, S_, N)
        Q = len(COVERAGES)
        outputs = (C_ + 1) * N * (K * 8 + 4) + N * (K + Q + 1) * 4 + (C_ + 1) * (5 + 2 * Q + 3 * N_BINS) * 8 + Q * 8
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
        rec = {'shape': name, 'net': [F, *hs], 'C': C_, 'S': S_, 'N': N, 'K': K, 'kernel': eng.grad_kernel, 'logit_bytes': C_ * S_ * N * K * 4,
               'workspace_bytes': ws, 'stream_s': min(t_new), 'stream_runs_s': t_new, 'stream_peak_bytes': max(m_new),
               'stream_peak_allowed_bytes': ws + outputs + inputs}
        assert rec['stream_peak_bytes'] <= rec['stream_peak_allowed_bytes'], rec
        if b is not None:
            rec.update(dense_s=min(t_old), dense_runs_s=t_old, dense_peak_bytes=max(m_old), speedup=min(t_old) / min(t_new))
            rec['max_diff_probs'] = float((a['probs'] - b['probs']).abs().max())
            for k in ('order', 'set_size', 'rank', 'kept'):                     # (two fp64 paths: a near-tie may fall either way)
                rec[f'differing_{k}'] = int((a[k] != b[k]).sum())
            rec['max_rel_diff_totals'] = float(((a['totals'] - b['totals']).abs() / b['totals'].abs().clamp(min=1.0)).max())
            del b
            raw, t_fwd, _ = once(predict_all)                                   # the parts: the forward alone, the calibration kernels alone
            _, t_cal, _ = once(lambda: eng.calibration(raw, y, COVERAGES, N_BINS))
            rec.update(predict_s=t_fwd, calibration_on_held_logits_s=t_cal)
            del raw
        print(json.dumps(rec), flush=True)
        del eng, theta, X, y, a


if __name__ == '__main__':
    main()
