"""mile_chain_diagnostics_tail and mile_multichain_ess on the GPU against the fp64 restatement tests/dtail_ref.py.

Tolerances come from yardsticks measured on the same inputs, never from the kernels' own output:
  each ESS      4 x the larger of (a) the error of the existing fp32 device path, mile_amd.diagnostics.effective_sample_size
                on the CUDA fp32 pieces of that series, and (b) the error of dtail_ref with its normal scores rounded to
                float32.  Cells where a Geyer pair sum up to the truncating one is below 1e-4 in dtail_ref (min_pair_mc) are
                left out (the estimator jumps there); at most 2 % of a shape's 4 * d cells.
  rhat_folded   4 x the relative error of a float32 NumPy evaluation of the same formula
  mcse_mean     4 x the larger of the raw series' ESS yardstick and the error of a float32 evaluation of the sd
quantiles are compared bit for bit.
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
import dtail_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
DEV = 'cuda:0'
OUTPUTS = ('ess_bulk', 'ess_tail', 'ess_mean', 'mcse_mean', 'rhat_folded')

#        C   S     d   ties   n_splits  path
SHAPES = [(3, 64, 40, False, 2, 'library'),
          (4, 250, 96, True, 2, 'library'),
          (2, 100, 70, True, 4, 'library'),
          (12, 1000, 16, False, 2, 'library'),
          (1, 128, 8, False, 2, 'library'),
          (2, 8, 8, False, 1, 'library'),
          (1, 4, 8, False, 2, 'library'),
          (16, 1024, 16, False, 2, 'library'),                # pooled n = 16 384: exactly the LDS bound
          (5, 3500, 16, False, 2, 'library+torch_sort')]      # pooled n = 17 500: past it


def _relerr(got, ref):
    m = np.isfinite(ref)
    if not m.any():
        return 0.0
    return float(np.max(np.abs(got[m] - ref[m]) / np.abs(ref[m])))


def _reference(x, ns):
    """fp64 reference, the kept ESS cells [4, d] and the float32 yardsticks of draws x [C, S, d]."""
    ref = T.tail_diagnostics(x, ns)
    ess4 = T.series_ess(x, ns)
    keep = T.series_min_pair(x, ns) >= 1e-4
    masked = lambda a: np.where(keep, a, np.nan)
    b4 = T.series_ess(x, ns, score_dtype=np.float32)
    y = {'b': [_relerr(masked(b4)[i], masked(ess4)[i]) for i in range(4)],
         'rhat_folded': _relerr(T.tail_diagnostics(x, ns, rhat_dtype=np.float32)['rhat_folded'], ref['rhat_folded'])}
    with np.errstate(all='ignore'):
        n = x.shape[0] * x.shape[1]
        y['sd'] = _relerr(x.reshape(n, -1).std(axis=0, ddof=1, dtype=np.float32).astype(np.float64), ref['sd'])
    return ref, ess4, keep, y


@functools.lru_cache(maxsize=None)
def _case(C_, S, d, ties, ns):
    """Input, reference and yardsticks of one shape (computed once, shared, never changed)."""
    x = R.ar1_draws(C_, S, d, 1, ties)
    ref, ess4, keep, y = _reference(x, ns)
    for v in (x, ess4, keep, *ref.values()):
        v.setflags(write=False)
    return x, ref, ess4, keep, y


def _yardstick_a(x, ns, ess4, keep):
    """The existing fp32 device path on the pieces of each series: [4] relative errors on the kept cells."""
    from mile_amd.diagnostics import effective_sample_size
    s = T.series(x)
    C_, S = x.shape[:2]
    out = []
    for i, k in enumerate(T.SERIES):
        pieces = torch.from_numpy(s[k].astype(np.float32).reshape(C_ * ns, S // ns, -1)).to(DEV)
        old = effective_sample_size(pieces).cpu().numpy().astype(np.float64).reshape(-1)
        out.append(_relerr(np.where(keep[i], old, np.nan), np.where(keep[i], ess4[i], np.nan)))
    return out


def _run(x, ns, plane=False, **kw):
    from mile_amd import metrics as M
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)) if plane else np.array(x)).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        out = M.tail_diagnostics(xt, ns, plane=plane, **kw)
    torch.cuda.synchronize()
    assert all(v.dtype == torch.float32 for v in out.values())
    return {k: (v.cpu().numpy() if k == 'quantiles' else v.cpu().numpy().astype(np.float64)) for k, v in out.items()}, M.LAST_DTAIL_PATH


def _check(got, ref, keep, y, ya, tag, cap=True):
    cell = {'ess_bulk': keep[0], 'ess_tail': keep[1] & keep[2], 'ess_mean': keep[3], 'mcse_mean': keep[3]}
    ess_y = [max(ya[i], y['b'][i]) for i in range(4)]
    bound = {'ess_bulk': 4 * ess_y[0], 'ess_tail': 4 * max(ess_y[1], ess_y[2]), 'ess_mean': 4 * ess_y[3],
             'mcse_mean': 4 * max(ess_y[3], y['sd']), 'rhat_folded': 4 * y['rhat_folded']}
    errs = {k: _relerr(np.where(cell[k], got[k], np.nan) if k in cell else got[k], np.where(cell[k], ref[k], np.nan) if k in cell else ref[k])
            for k in OUTPUTS}
    print(f'DTAIL {tag}: ess cells left out {int((~keep).sum())}/{keep.size}  yardstick a {["%.2e" % v for v in ya]} b {["%.2e" % v for v in y["b"]]}  ' +
          '  '.join(f'{k} err {errs[k]:.3e} bound {bound[k]:.3e}' for k in errs))
    assert got['quantiles'].dtype == np.float32 and np.array_equal(got['quantiles'], ref['quantiles'], equal_nan=True), (tag, 'quantiles')
    for k in OUTPUTS:
        assert (np.isnan(got[k]) == np.isnan(ref[k])).all(), (tag, k, 'NaN pattern')
    if cap:
        assert (~keep).sum() <= 0.02 * keep.size
    for k in errs:
        assert errs[k] <= bound[k], (tag, k, errs[k], bound[k])


@pytest.mark.parametrize('plane', [False, True], ids=['draws', 'plane'])
@pytest.mark.parametrize('C_,S,d,ties,ns,path', SHAPES)
def test_matches_the_restatement(C_, S, d, ties, ns, path, plane):
    x, ref, ess4, keep, y = _case(C_, S, d, ties, ns)
    got, ran = _run(x, ns, plane)
    assert ran == path
    assert all(got[k].shape == (d,) for k in OUTPUTS) and got['quantiles'].shape == (3, d)
    _check(got, ref, keep, y, _yardstick_a(x, ns, ess4, keep), f'{(C_, S, d, ties, ns, plane)}')
    if (C_, S) == (1, 4):
        assert np.isnan(got['ess_tail']).all()                      # I_hi is all ones at n = 4


def test_one_unsplit_chain_ties_with_the_single_chain_kernels():
    """C = 1, n_splits = 1: ESS_mc is the single-chain estimator, so ess_bulk is mile_chain_diagnostics' ess[0], both fp64
    evaluations of one quantity rounded once: within 1 fp32 ulp on the kept cells."""
    from mile_amd import metrics as M
    x = R.ar1_draws(1, 128, 8, 1, False)
    keep = T.series_min_pair(x, 1)[0] >= 1e-4
    got, _ = _run(x, 1)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        old = M.chain_diagnostics(torch.from_numpy(x).to(DEV), 1)['ess'][0].cpu().numpy()
    new = got['ess_bulk'].astype(np.float32)
    assert keep.sum() >= 6
    assert (np.abs(new[keep] - old[keep]) <= np.spacing(np.maximum(np.abs(new[keep]), np.abs(old[keep])))).all(), (new, old)


@pytest.mark.parametrize('C_,S,d,ties,ns', [s[:5] for s in SHAPES[:5]])
def test_score_planes_are_those_of_the_pooled_ranking_kernel(C_, S, d, ties, ns):
    """The round trip through mile_chain_diagnostics: its k_diag_pool_rank ranks the folded draws (folded here in fp32, as
    stated), its k_diag_chain / k_diag_final give their split R-hat.  rhat_folded comes from the same two kernels on the score
    plane k_dtail_derive wrote, so the two agree bit for bit only if that plane holds k_diag_pool_rank's scores."""
    from mile_amd import metrics as M
    x = _case(C_, S, d, ties, ns)[0]
    got, _ = _run(x, ns)
    f = np.abs(x - got['quantiles'][2])
    assert f.dtype == np.float32
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        rt = M.chain_diagnostics(torch.from_numpy(f).to(DEV), ns)['rhat'].cpu().numpy()
    assert np.array_equal(rt.astype(np.float64), got['rhat_folded'], equal_nan=True)


def test_torch_sort_path_under_the_bound_agrees_with_the_library_path():
    C_, S, d, ties, ns = 4, 250, 96, True, 2
    x, ref, ess4, keep, y = _case(C_, S, d, ties, ns)
    lib, p0 = _run(x, ns)
    ts, p1 = _run(x, ns, torch_sort=True)
    assert (p0, p1) == ('library', 'library+torch_sort')
    for k in ('ess_tail', 'ess_mean', 'quantiles'):                 # the same kernel on the same input
        assert np.array_equal(lib[k], ts[k], equal_nan=True), k
    _check(ts, ref, keep, y, _yardstick_a(x, ns, ess4, keep), 'forced torch sort')
    assert _relerr(np.where(keep[0], ts['ess_bulk'], np.nan), np.where(keep[0], lib['ess_bulk'], np.nan)) <= 4 * y['b'][0]
    assert _relerr(ts['rhat_folded'], lib['rhat_folded']) <= 4 * y['rhat_folded']
    assert _relerr(ts['mcse_mean'], lib['mcse_mean']) <= 4 * y['sd']


def test_multichain_ess_of_given_series():
    """mile_multichain_ess alone, both layouts, against the restatement on the raw draws."""
    from mile_amd import metrics as M
    C_, S, d, ties, ns = 2, 100, 70, True, 4
    x, ref, ess4, keep, y = _case(C_, S, d, ties, ns)
    ya = _yardstick_a(x, ns, ess4, keep)
    a = M.multichain_ess(torch.from_numpy(np.array(x)).to(DEV), ns).cpu().numpy().astype(np.float64)
    b = M.multichain_ess(torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1))).to(DEV), ns, plane=True).cpu().numpy().astype(np.float64)
    assert np.array_equal(a, b)
    assert _relerr(np.where(keep[3], a, np.nan), np.where(keep[3], ess4[3], np.nan)) <= 4 * max(ya[3], y['b'][3])
    got, _ = _run(x, ns)
    assert np.array_equal(a, got['ess_mean'])


def test_non_finite_draws_ties_at_the_threshold_and_a_constant_column():
    C_, S, d, ties, ns = 3, 64, 40, False, 2
    x0, ref0, ess40, keep0, y0 = _case(C_, S, d, ties, ns)
    x = x0.copy()
    x[1, 17, 5] = np.nan
    x[0, 30, 9] = np.inf
    x[2, 3, 11] = -np.inf
    x[:, :, 20] = -0.75                                              # constant
    col = x[:, :, 14].reshape(-1)
    col[np.argsort(col)[:20]] = np.sort(col)[19]                     # a tie group over sorted positions 0 .. 19; q_lo is position 9
    x[:, :, 14] = col.reshape(C_, S)
    with np.errstate(all='ignore'):
        ref, ess4, keep, y = _reference(x, ns)
    base, _ = _run(x0, ns)
    got, _ = _run(x, ns)
    other = np.ones(d, bool)
    other[[5, 9, 11, 14, 20]] = False
    for k in got:                                                    # every other column: bit for bit what it was
        assert np.array_equal(got[k][..., other], base[k][..., other], equal_nan=True), k
    _check(got, ref, keep, y, _yardstick_a(x, ns, ess4, keep), 'nan/inf/ties/constant', cap=False)
    assert all(np.isnan(got[k][5]) for k in OUTPUTS) and np.isnan(got['quantiles'][:, 5]).all()
    assert all(np.isnan(got[k][20]) for k in OUTPUTS) and (got['quantiles'][:, 20] == -0.75).all()
    for c in (9, 11):
        assert np.isnan(got['ess_mean'][c]) and np.isnan(got['mcse_mean'][c])
        assert np.isfinite(got['ess_bulk'][c]) and np.isfinite(got['ess_tail'][c]) and np.isfinite(got['rhat_folded'][c])
    assert int((x[:, :, 14] <= got['quantiles'][0, 14]).sum()) == 20 and np.isfinite(got['ess_tail'][14])


def test_argument_errors_launch_nothing():
    from mile_amd import _lib
    lib = _lib.load_library()
    B = _lib.DTAIL_BITS
    every = B['ess_bulk'] | B['ess_tail'] | B['ess_mean'] | B['rhat_folded']
    src = torch.zeros(5000 * 4, device=DEV)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=DEV)
    outs = [torch.full((64,), -7.0, device=DEV) for _ in range(5)]
    quant = torch.full((3 * 64,), -7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(C_, S, d, ns, what=every, nbytes=ws.numel(), source=src, o=outs, q=quant):
        return lib.mile_chain_diagnostics_tail(p(source), C_, S, d, ns, what, *[p(t) for t in o], p(q), p(ws), nbytes, None)

    assert call(3, 64, 4, 2, source=None) == -1
    assert call(0, 64, 4, 2) == -1 and call(65536, 64, 4, 2) == -1
    assert call(3, 2, 4, 2) == -1 and call(1, 5000, 4, 2) == -1 and call(3, 64, 0, 2) == -1
    assert call(3, 64, 4, 3) == -1 and call(3, 64, 4, 0) == -1 and call(3, 64, 4, 64) == -1
    assert call(3, 64, 4, 2, what=0) == -1 and call(3, 64, 4, 2, what=B['plane_input']) == -1 and call(3, 64, 4, 2, what=every | 32) == -1
    for i in range(5):                                              # a null pointer for an output asked for
        assert call(3, 64, 4, 2, o=[None if j == i else t for j, t in enumerate(outs)]) == -1
    need = lib.mile_chain_diagnostics_tail_workspace(3, 64, 4, every)
    assert need > 0 and lib.mile_chain_diagnostics_tail_workspace(3, 2, 4, every) == -1
    assert call(3, 64, 4, 2, nbytes=need - 1) == -2
    for what in (B['ess_bulk'], B['ess_tail'], B['rhat_folded']):   # past the pooled bound: everything that needs the sort
        assert call(5, 3500, 1, 2, what=what) == -1 and b'unsupported' in lib.mile_last_error()
    assert call(5, 3500, 1, 2, what=B['ess_mean']) == -1 and b'unsupported' in lib.mile_last_error()      # (quantiles asked for)
    ess = torch.full((64,), -7.0, device=DEV)
    mc = lambda C_, S, m, ns, plane=0, nbytes=ws.numel(), source=src, e=ess: lib.mile_multichain_ess(p(source), C_, S, m, ns, plane, p(e),
                                                                                                     p(ws), nbytes, None)
    assert mc(3, 64, 4, 2, source=None) == -1 and mc(3, 64, 4, 2, e=None) == -1
    assert mc(3, 2, 4, 2) == -1 and mc(3, 64, 4, 3) == -1 and mc(3, 64, 4, 64) == -1
    assert mc(3, 64, 4, 2, nbytes=lib.mile_multichain_ess_workspace(3, 64, 4, 0) - 1) == -2
    assert lib.mile_multichain_ess_workspace(3, 64, 4, 1) == 0 and lib.mile_multichain_ess_workspace(3, 2, 4, 0) == -1
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs + [quant, ess]) and not bool(ws.any())
    assert call(3, 64, 4, 2, nbytes=need) == 0                      # the same call with enough workspace runs
    assert call(5, 3500, 1, 2, what=B['ess_mean'], q=None) == 0     # the raw series needs no sort: it runs past the bound
    torch.cuda.synchronize()
    assert not bool((outs[0][:4] == -7.0).any()) and bool((outs[0][4:] == -7.0).all())
    assert not bool((quant[:12] == -7.0).any()) and bool((quant[12:] == -7.0).all())     # [3][d], d = 4


def test_deterministic_and_chunked_walk_agree():
    """Two calls are bitwise equal; so is a call whose workspace holds one 32-parameter tile at a time (3 chunks for 70), in
    both layouts."""
    from mile_amd import _lib
    lib = _lib.load_library()
    C_, S, d, ns = 2, 100, 70, 4
    x = _case(C_, S, d, True, ns)[0]
    a, _ = _run(x, ns)
    b, _ = _run(x, ns)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    B = _lib.DTAIL_BITS
    p = lambda t: C.c_void_p(t.data_ptr())
    for plane in (False, True):
        what = B['ess_bulk'] | B['ess_tail'] | B['ess_mean'] | B['rhat_folded'] | (B['plane_input'] if plane else 0)
        xt = torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)) if plane else np.array(x)).to(DEV)
        per = lib.mile_chain_diagnostics_tail_workspace(C_, S, 1, what)
        ws = torch.empty(32 * per, dtype=torch.uint8, device=DEV)
        o = {k: torch.empty(d, device=DEV) for k in OUTPUTS}
        o['quantiles'] = torch.empty((3, d), device=DEV)
        rc = lib.mile_chain_diagnostics_tail(p(xt), C_, S, d, ns, what, *[p(o[k]) for k in OUTPUTS], p(o['quantiles']), p(ws), ws.numel(), None)
        assert rc == 0, lib.mile_last_error()
        torch.cuda.synchronize()
        for k in a:
            assert np.array_equal(a[k], o[k].cpu().numpy().astype(a[k].dtype), equal_nan=True), (k, plane)


def test_function_space_columns():
    """fdiag_tail_* of evaluate.py are tail_diagnostics(columns, plane=True) of the columns mile_function_diagnostics returns, the
    summed log-likelihood's column included."""
    from oracle import mclmc_oracle as O
    from mile_amd import ModelSpec
    from mile_amd import metrics as M
    from mile_amd.engine import Engine
    import evaluate as E
    C_, S, N = 3, 64, 9
    ospec = O.ModelSpec(5, (8, 2), activation='tanh', task='regr')
    prob = O.synthetic_problem(ospec, 32, C_ * S, seed=3, theta_scale=0.3)
    test = O.synthetic_problem(ospec, N, 1, seed=4)
    eng = Engine(ModelSpec(5, (8, 2), activation='tanh', task='regr'), torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV)
    theta = prob['theta0'].reshape(C_, S, -1).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        keys, arrays, (tkeys, tarrays) = E.function_diagnostic_metrics(eng, theta, test['X'][:N], test['y'][:N], 'regr', 2, 2)
        res = eng.function_diagnostics(torch.from_numpy(theta), torch.from_numpy(test['X'][:N]), torch.from_numpy(test['y'][:N]),
                                       n_splits=2, return_columns=True)
        tail = M.tail_diagnostics(res['columns'], 2, plane=True)
        want, _ = E.tail_keys('fdiag_tail', tail, C_ * S, 2, res['rhat'])
    Mcols = N * 3 + 1
    assert res['columns'].shape == (Mcols, C_, S) and M.LAST_DTAIL_PATH == 'library'
    for k in OUTPUTS + ('quantiles',):
        assert tarrays['fdiag_' + k].shape[-1] == Mcols
        assert np.array_equal(tarrays['fdiag_' + k], tail[k].cpu().numpy(), equal_nan=True), k
    assert tkeys == want and all(np.isfinite(v) for v in tkeys.values())
    # and the columns' statistics are those of the restatement's NaN pattern: every column finite here
    ref = T.tail_diagnostics(res['columns'].permute(1, 2, 0).cpu().numpy(), 2)
    for k in OUTPUTS:
        assert (np.isnan(tail[k].cpu().numpy()) == np.isnan(ref[k])).all(), k
    assert np.array_equal(tail['quantiles'].cpu().numpy(), ref['quantiles'])


def test_evaluate_cli_tail_diagnostics(tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=80, n_chains=4)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, str(ROOT / 'train.py'), '-c', str(tmp_path / 'cfg.yaml'), '-d', '1'],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp = tmp_path / 'smoke_synthetic'
    names = ('n_splits', 'ess_bulk_min', 'ess_bulk_median', 'ess_tail_min', 'ess_tail_median', 'rhat_folded_median', 'rhat_folded_max',
             'rhat_rank_max', 'mcse_mean_over_sd_max', 'ess_bulk_share')

    def evaluate(*flags):
        r = subprocess.run([sys.executable, str(ROOT / 'evaluate.py'), '-e', str(exp), *flags], capture_output=True, text=True,
                           cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return json.loads((exp / 'metrics.json').read_text())

    three = ('--diagnostics', '--function-diagnostics', '--canonical-diagnostics')
    before = evaluate(*three)
    assert not any('tail' in k for k in before) and not (exp / 'tail_diagnostics.npz').exists()
    m = evaluate('--tail-diagnostics')
    C_, S = m['n_chains'], m['n_samples']
    z = np.load(exp / 'tail_diagnostics.npz')
    d = z['ess_bulk'].shape[0]
    assert set(z.files) == set(OUTPUTS) | {'quantiles'} and z['quantiles'].shape == (3, d)
    assert all(z[k].shape == (d,) and np.isfinite(z[k]).all() for k in OUTPUTS)
    assert m['dtail_n_splits'] == 2 and all(np.isfinite(m['dtail_' + k]) for k in names)
    assert abs(m['dtail_ess_bulk_share'] - float(np.median(z['ess_bulk'])) / (C_ * S)) < 1e-6
    assert not any(k.startswith(('fdiag_tail_', 'cdiag_tail_', 'diag_')) for k in m)
    both = evaluate(*three, '--tail-diagnostics')
    for pre in ('dtail_', 'fdiag_tail_', 'cdiag_tail_'):
        assert all(np.isfinite(both[pre + k]) for k in names), pre
    z = np.load(exp / 'tail_diagnostics.npz')
    assert z['cdiag_ess_bulk'].shape == (d,) and z['fdiag_ess_bulk'].shape[0] == np.load(exp / 'function_diagnostics.npz')['rhat'].shape[0]
    for k, v in before.items():                                     # every key the three flags wrote before is unchanged
        if k.startswith(('diag_', 'fdiag_', 'cdiag_')):
            assert both[k] == v or (isinstance(v, float) and np.isnan(v) and np.isnan(both[k])), k
    assert all(both['dtail_' + k] == m['dtail_' + k] for k in names)
