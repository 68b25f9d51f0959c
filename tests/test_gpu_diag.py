"""mile_chain_diagnostics on the GPU against the fp64 restatement tests/diag_ref.py.

Tolerances come from yardsticks measured on the same inputs, never from the kernels' own output:
  ess           4 x the larger of (a) the error of the existing device path (mile_amd.metrics.effective_sample_size on a
                CUDA fp32 tensor, computed here at run time) and (b) the error of diag_ref with its normal scores rounded
                to float32.  Cells where a Geyer pair sum up to the truncating one is below 1e-4 in diag_ref are left out
                (the estimator jumps there); at most 2 % of a shape's cells.
  wcv, bcv      4 x the error of a float32 NumPy evaluation of diag_ref's formulas, relative to wcv
  crhat, rhat   4 x the relative error of the same float32 evaluation
"""
import ctypes as C
import functools
import json
import subprocess
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import diag_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
DEV = 'cuda:0'

#        C   S     d   ties   n_splits  path
SHAPES = [(3, 64, 40, False, 2, 'library'),
          (4, 250, 96, True, 2, 'library'),
          (2, 100, 70, True, 4, 'library'),
          (12, 1000, 16, False, 2, 'library'),
          (1, 128, 8, False, 2, 'library'),
          (16, 1024, 8, False, 2, 'library'),                 # pooled n = 16 384: exactly the LDS bound
          (5, 3500, 8, False, 2, 'library+torch_sort')]       # pooled n = 17 500: past it


def _relerr(got, ref, scale=None):
    m = np.isfinite(ref)
    if not m.any():
        return 0.0
    s = np.abs(ref if scale is None else np.broadcast_to(scale, ref.shape))
    return float(np.max(np.abs(got[m] - ref[m]) / s[m]))


@functools.lru_cache(maxsize=None)
def _case(C_, S, d, ties, ns):
    """Input, fp64 reference, ESS mask and the float32 yardsticks of one shape (computed once, shared, never changed)."""
    x = R.ar1_draws(C_, S, d, 1, ties)
    ref = R.chain_diagnostics(x, ns)
    keep = R.geyer_min_pair(x) >= 1e-4
    x32 = x.astype(np.float32)
    with np.errstate(all='ignore'):
        y = {'wcv': _relerr(R.within_chain_var(x32).astype(np.float64), ref['wcv'], ref['wcv']),
             'bcv': _relerr(R.between_chain_var(x32).astype(np.float64), ref['bcv'], ref['wcv']),
             'crhat': _relerr(R.split_chain_r_hat(x, ns, dtype=np.float32).astype(np.float64), ref['crhat']),
             'rhat': _relerr(R.gelman_split_r_hat(x, ns, dtype=np.float32).astype(np.float64), ref['rhat'])}
    ess_b = R.effective_sample_size(x, score_dtype=np.float32)
    y['ess_b'] = _relerr(np.where(keep, ess_b, np.nan), np.where(keep, ref['ess'], np.nan))
    for v in (x, keep, *ref.values()):
        v.setflags(write=False)
    return x, ref, keep, y


def _run(x, ns):
    from mile_amd import metrics as M
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        out = M.chain_diagnostics(torch.from_numpy(x).to(DEV), ns)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().astype(np.float64) for k, v in out.items()}, M.LAST_DIAG_PATH


def _check(got, ref, keep, y, ya, tag):
    errs = {'wcv': _relerr(got['wcv'], ref['wcv'], ref['wcv']), 'bcv': _relerr(got['bcv'], ref['bcv'], ref['wcv']),
            'crhat': _relerr(got['crhat'], ref['crhat']), 'rhat': _relerr(got['rhat'], ref['rhat']),
            'ess': _relerr(np.where(keep, got['ess'], np.nan), np.where(keep, ref['ess'], np.nan))}
    bound = {k: 4 * y[k] for k in ('wcv', 'bcv', 'crhat', 'rhat')}
    bound['ess'] = 4 * max(ya, y['ess_b'])
    print(f'DIAG {tag}: ess left out {int((~keep).sum())}/{keep.size}  yardstick a {ya:.3e} b {y["ess_b"]:.3e}  ' +
          '  '.join(f'{k} err {errs[k]:.3e} bound {bound[k]:.3e}' for k in errs))
    for k in ('wcv', 'bcv', 'ess', 'crhat', 'rhat'):
        assert (np.isnan(got[k]) == np.isnan(ref[k])).all(), (tag, k, 'NaN pattern')
    assert (~keep).sum() <= 0.02 * keep.size
    for k in errs:
        assert errs[k] <= bound[k], (tag, k, errs[k], bound[k])


def _yardstick_a(x, ref, keep):
    """The existing fp32 device path on the same cells."""
    from mile_amd.metrics import effective_sample_size
    old = effective_sample_size(torch.from_numpy(x).to(DEV)).cpu().numpy().astype(np.float64)
    return _relerr(np.where(keep, old, np.nan), np.where(keep, ref['ess'], np.nan))


@pytest.mark.parametrize('C_,S,d,ties,ns,path', SHAPES)
def test_matches_the_restatement(C_, S, d, ties, ns, path):
    x, ref, keep, y = _case(C_, S, d, ties, ns)
    got, ran = _run(x, ns)
    assert ran == path
    assert got['ess'].shape == got['crhat'].shape == (C_, d) and got['rhat'].shape == got['wcv'].shape == got['bcv'].shape == (d,)
    _check(got, ref, keep, y, _yardstick_a(x, ref, keep), f'{(C_, S, d, ties, ns)}')
    if C_ == 1:
        assert np.isnan(got['bcv']).all() and np.isfinite(got['rhat']).all()


def test_non_finite_draws():
    C_, S, d, ties, ns = 3, 64, 40, False, 2
    x0, ref0, keep0, y = _case(C_, S, d, ties, ns)
    x = x0.copy()
    x[1, 17, 5] = np.nan
    x[0, 30, 9] = np.inf
    ref = R.chain_diagnostics(x, ns)
    base, _ = _run(x0, ns)
    got, _ = _run(x, ns)
    other = np.ones(d, bool)
    other[[5, 9]] = False
    for k in got:                                   # every other column: bit for bit what it was
        assert np.array_equal(got[k][..., other], base[k][..., other], equal_nan=True), k
    keep = R.geyer_min_pair(np.nan_to_num(x, nan=0.0, posinf=1e30)) >= 1e-4
    keep[:, 5] = True                               # all-NaN scores: no pair sum is positive, the ESS is its floor
    keep[:, other] = keep0[:, other]
    _check(got, ref, keep, y, _yardstick_a(x0, ref0, keep0), 'nan/inf')
    assert np.isnan(got['rhat'][5]) and np.isnan(got['crhat'][1, 5]) and np.isfinite(got['crhat'][[0, 2], 5]).all()
    assert np.isfinite(got['rhat'][9]) and np.isfinite(got['crhat'][:, 9]).all() and np.isnan(got['wcv'][9])


def test_tie_groups_share_one_score():
    """Two chains that hold the same tied values in the same order have identical scores only if tied draws share a rank:
    then the between-part of rhat (n_splits = 1) is exactly 0 and rhat = sqrt((S - 1) / S)."""
    v = np.array([0, 0, 1, 1, 1, 2, 3, 3], np.float32)
    x = np.stack([v, v])[:, :, None].copy()
    got, _ = _run(x, 1)
    assert abs(got['rhat'][0] - np.sqrt(7 / 8)) < 1e-6
    ref = R.chain_diagnostics(x, 1)
    assert abs(ref['rhat'][0] - np.sqrt(7 / 8)) < 1e-12
    # and on a shape with rounded columns every tied column agrees with scipy's average ranks
    xt, reft, _, y = _case(4, 250, 96, True, 2)
    gt, _ = _run(xt, 2)
    tied = np.arange(96) % 4 == 0
    assert _relerr(gt['rhat'][tied], reft['rhat'][tied]) <= 4 * y['rhat']
    assert _relerr(gt['crhat'][:, tied], reft['crhat'][:, tied]) <= 4 * y['crhat']


def test_argument_errors_launch_nothing():
    from mile_amd import _lib
    lib = _lib.load_library()
    B = _lib.DIAG_BITS
    every = B['wcv'] | B['bcv'] | B['ess'] | B['crhat'] | B['rhat']
    src = torch.zeros(5000 * 4, device=DEV)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)
    outs = [torch.full((64,), -7.0, device=DEV) for _ in range(5)]
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(C_, S, d, ns, nbytes=ws.numel()):
        return lib.mile_chain_diagnostics(p(src), C_, S, d, ns, every, *[p(o) for o in outs], p(ws), nbytes, None)

    assert call(3, 64, 4, 3) == -1
    assert call(3, 2, 4, 2) == -1
    assert call(1, 5000, 4, 2) == -1
    need = lib.mile_chain_diagnostics_workspace(3, 64, 4, every)
    assert call(3, 64, 4, 2, need - 1) == -2
    assert call(5, 3500, 1, 2) == -1 and b'unsupported' in lib.mile_last_error()
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs) and not bool(ws.any())
    assert call(3, 64, 4, 2, need) == 0                    # the same call with enough workspace runs
    torch.cuda.synchronize()
    assert not bool((outs[0][:4] == -7.0).any()) and bool((outs[0][4:] == -7.0).all())
    assert not bool((outs[2][:12] == -7.0).any()) and bool((outs[2][12:] == -7.0).all())


def test_deterministic_and_chunked_walk_agree():
    """Two calls are bitwise equal; so is a call whose workspace holds one 32-parameter tile at a time (3 chunks for 70)."""
    from mile_amd import _lib
    lib = _lib.load_library()
    x, *_ = _case(2, 100, 70, True, 4)
    a, _ = _run(x, 4)
    b, _ = _run(x, 4)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    B = _lib.DIAG_BITS
    every = B['wcv'] | B['bcv'] | B['ess'] | B['crhat'] | B['rhat']
    xt = torch.from_numpy(x).to(DEV)
    per = lib.mile_chain_diagnostics_workspace(2, 100, 1, every)
    ws = torch.empty(32 * per, dtype=torch.uint8, device=DEV)
    o = {k: torch.empty((2, 70) if k in ('ess', 'crhat') else (70,), device=DEV) for k in ('wcv', 'bcv', 'ess', 'crhat', 'rhat')}
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = lib.mile_chain_diagnostics(p(xt), 2, 100, 70, 4, every, *[p(o[k]) for k in ('wcv', 'bcv', 'ess', 'crhat', 'rhat')],
                                    p(ws), ws.numel(), None)
    assert rc == 0, lib.mile_last_error()
    torch.cuda.synchronize()
    for k in a:
        assert np.array_equal(a[k], o[k].cpu().numpy().astype(np.float64), equal_nan=True), k


def test_evaluate_cli_diagnostics(tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=80, n_chains=4)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, str(ROOT / 'train.py'), '-c', str(tmp_path / 'cfg.yaml'), '-d', '1'],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp = tmp_path / 'smoke_synthetic'
    r = subprocess.run([sys.executable, str(ROOT / 'evaluate.py'), '-e', str(exp), '--diagnostics'], capture_output=True,
                       text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = json.loads((exp / 'metrics.json').read_text())
    C_, S = m['n_chains'], m['n_samples']
    z = np.load(exp / 'diagnostics.npz')
    d = z['rhat'].shape[0]
    assert z['ess'].shape == z['crhat'].shape == (C_, d) and z['wcv'].shape == z['bcv'].shape == (d,) and S >= 4
    assert all(np.isfinite(z[k]).all() for k in ('ess', 'crhat', 'rhat', 'wcv', 'bcv'))
    assert m['diag_n_splits'] == 2
    for k in ('diag_ess_min', 'diag_ess_median', 'diag_crhat_median', 'diag_crhat_max', 'diag_rhat_median', 'diag_rhat_max',
              'diag_wcv_median', 'diag_bcv_median'):
        assert np.isfinite(m[k]), k
    assert sum(len(v) for v in (m['diag_ess_layer_mean'], m['diag_crhat_layer_mean'])) >= 2
    assert abs(m['diag_ess_min'] - float(z['ess'].min())) < 1e-6 * abs(m['diag_ess_min'])
    r = subprocess.run([sys.executable, str(ROOT / 'evaluate.py'), '-e', str(exp)], capture_output=True, text=True, cwd=ROOT,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert not any(k.startswith('diag_') for k in json.loads((exp / 'metrics.json').read_text()))


def test_chain_lengths_the_kernels_do_not_take_run_in_torch_and_say_so():
    from mile_amd import metrics as M
    x = R.ar1_draws(2, 4200, 3, 1, False)
    with pytest.warns(UserWarning, match='outside the range of the HIP kernels'):
        got = M.chain_diagnostics(torch.from_numpy(x).to(DEV), 2)
    assert M.LAST_DIAG_PATH == 'torch'
    ref = R.chain_diagnostics(x, 2)
    for k in ('wcv', 'bcv', 'crhat', 'rhat'):                    # fp64 torch, as tests/test_diag_host.py checks on the CPU
        np.testing.assert_allclose(got[k].cpu().numpy(), ref[k], rtol=1e-9)
    assert got['ess'].shape == (2, 3) and bool(torch.isfinite(got['ess']).all())
