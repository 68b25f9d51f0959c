"""Tail-diagnostics timing: mile_amd.metrics.tail_diagnostics (mile_chain_diagnostics_tail; past the pooled bound torch sorts
plus mile_multichain_ess) against the torch fp32 FFT form of the same outputs: the series by torch sorts
(metrics.tail_series_dense), mile_amd.diagnostics.effective_sample_size on the CUDA fp32 pieces of the four series, the split
R-hat of the folded scores in torch, columns in chunks that keep the fp64 sort keys under 256 MB.

    python tools/dtail_time.py [--reps 3] [--shapes stock b2]

Shapes: [12, 1000, 402] (stock net) and [128, 1000, 8834] (B2), synthetic AR(1) draws generated on the device as in
tools/diag_time.py.  Host clock around work that ends in a device synchronise, best of `reps` after one warm-up call; peak
memory is torch's allocator's, above the draws themselves.  One JSON line per shape.
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from mile_amd import metrics as M
from mile_amd.diagnostics import effective_sample_size as ess_fft

SHAPES = {'stock': (12, 1000, 402), 'b2': (128, 1000, 8834)}


def ar1(C, S, d, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    phi = torch.rand(d, generator=g, device=dev) * 1.48 - 0.5
    x = torch.empty((C, S, d), device=dev)
    x[:, 0] = torch.randn((C, d), generator=g, device=dev) / torch.sqrt(1 - phi ** 2)
    for t in range(1, S):
        x[:, t] = phi * x[:, t - 1] + torch.randn((C, d), generator=g, device=dev)
    return x + 0.3 * torch.randn((C, 1, d), generator=g, device=dev)


def torch_form(x, ns):
    """The five outputs from torch alone, fp32 FFT autocovariances."""
    C, S, d = x.shape
    out = {k: torch.empty(d, device=x.device) for k in M.TAIL_OUTPUTS}
    step = max(1, (1 << 28) // (C * S * 8))
    pieces = lambda v: v.to(torch.float32).reshape(C * ns, S // ns, -1)
    for k0 in range(0, d, step):
        xk = x[:, :, k0:k0 + step].contiguous()
        sl = slice(k0, k0 + xk.shape[2])
        ser = M.tail_series_dense(xk)
        out['ess_bulk'][sl] = ess_fft(pieces(ser['z']))
        out['ess_tail'][sl] = torch.minimum(ess_fft(pieces(ser['i_lo'])), ess_fft(pieces(ser['i_hi'])))
        out['ess_mean'][sl] = ess_fft(pieces(xk))
        out['mcse_mean'][sl] = xk.reshape(C * S, -1).std(dim=0, unbiased=True) / torch.sqrt(out['ess_mean'][sl])
        out['rhat_folded'][sl] = M._split_r_hat_of_scores(ser['zf'], ns).to(torch.float32)
    return out


def best(fn, reps):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', nargs='+', default=['stock', 'b2'], choices=sorted(SHAPES))
    ap.add_argument('--skip-torch', action='store_true', help='time the library path only (for a profiler run)')
    args = ap.parse_args()
    dev = 'cuda:0'
    for name in args.shapes:
        C, S, d = SHAPES[name]
        x = ar1(C, S, d, 1, dev)
        t_lib, m_lib = best(lambda: M.tail_diagnostics(x, 2), args.reps)
        rec = {'shape': name, 'C': C, 'S': S, 'd': d, 'path': M.LAST_DTAIL_PATH, 'library_s': t_lib, 'library_us_per_col': 1e6 * t_lib / d,
               'library_peak_mib': m_lib}
        if not args.skip_torch:
            t_old, m_old = best(lambda: torch_form(x, 2), max(1, args.reps - 1))
            new, old = M.tail_diagnostics(x, 2), torch_form(x, 2)
            rec.update(torch_s=t_old, torch_us_per_col=1e6 * t_old / d, torch_peak_mib=m_old, speedup=t_old / t_lib,
                       median_rel_diff={k: float(((new[k] - old[k]).abs() / old[k].abs()).nanmedian()) for k in M.TAIL_OUTPUTS})
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
