"""mile_function_diagnostics on the GPU (-m gpu).

Columns: mu and log sigma are the floats of Engine.predict (the same launch), bit for bit; every column against the fp64
restatement tests/fdiag_ref.py at the project's bound for these forward kernels, max|got - ref| < 1e-4 * max(1, max|ref|)
(tests/test_gpu_predict.py); loglik_sum at that bound times N.  Statistics: device-vs-fp64 forward error is kept out of the
comparison -- the five outputs must equal, bit for bit, metrics.chain_diagnostics (the library path, pinned against fp64 and
against chunking by tests/test_gpu_diag.py) of the returned columns.  Summaries: the fdiag_ref restatement of the device's own
statistic arrays; indices and counts exactly, means to 1e-12."""
import ctypes as C
import functools
import json
import subprocess
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import diag_ref as R
from tests import fdiag_ref as F
from tests import lenetti_ref as RL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ROOT = Path(__file__).resolve().parents[1]
DEV = 'cuda:0'
FIVE = ('wcv', 'bcv', 'ess', 'crhat', 'rhat')


@functools.lru_cache(maxsize=None)
def _fcn_case(F_, hs, act, task, C_, S, N, seed=3, theta_scale=0.3):
    """Draws [C, S, d], rows, labels and the fp64 columns of one FCN shape (computed once, shared, never changed)."""
    ospec = O.ModelSpec(F_, hs, activation=act, task=task)
    prob = O.synthetic_problem(ospec, 32, C_ * S, seed=seed, theta_scale=theta_scale)
    test = O.synthetic_problem(ospec, max(N, 4), 1, seed=seed + 1)          # (its labels are standardised: not from one row)
    test = {k: test[k][:N].copy() for k in ('X', 'y')}
    out = O.mlp_forward(ospec, prob['theta0'].astype(np.float64), test['X'].astype(np.float64)).reshape(C_, S, N, hs[-1])
    cols, L = F.columns(out, test['y'], task)
    cols_x, _ = F.columns(out, None, task)
    theta = prob['theta0'].reshape(C_, S, -1)
    for v in (theta, test['X'], test['y'], cols, L, cols_x):
        v.setflags(write=False)
    return ospec, prob, theta, test['X'], test['y'], cols, L, cols_x


def _fcn_engine(ospec, prob, kernel='auto'):
    from mile_amd import ModelSpec
    from mile_amd.engine import Engine
    spec = ModelSpec(ospec.in_features, ospec.hidden_structure, activation=ospec.activation, task=ospec.task)
    eng = Engine(spec, torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV, grad_kernel=kernel)
    assert kernel == 'auto' or eng.grad_kernel == kernel
    return eng


def _t(a):
    return torch.from_numpy(np.array(a))                  # a copy: the shared cases are read-only


def _np(res):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}


def _chain_diag(columns, ns):
    """metrics.chain_diagnostics (CUDA fp32: the library's kernels) of columns [M, C, S] as [C, S, M]."""
    from mile_amd import metrics as M
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        out = M.chain_diagnostics(columns.permute(1, 2, 0).contiguous(), ns)
    return {k: v.cpu().numpy() for k, v in out.items()}, M.LAST_DIAG_PATH


def _check(tag, eng, theta, X, y, task, ref_cols, ref_L, ns, **caps):
    """Run the call and hold columns, statistics and summaries against their yardsticks; returns the result as NumPy."""
    C_, S = theta.shape[:2]
    N, O_ = X.shape[0], eng.spec.hidden_structure[-1]
    raw = eng.function_diagnostics(_t(theta), _t(X), None if y is None else _t(y), n_splits=ns, return_columns=True, **caps)
    torch.cuda.synchronize()
    res = _np(raw)
    Q = O_ + (y is not None)
    M_ = N * Q + (y is not None)
    assert (res['Q'], res['M']) == (Q, M_) and res['columns'].shape == (M_, C_, S)
    assert res['ess'].shape == res['crhat'].shape == (C_, M_) and res['rhat'].shape == res['wcv'].shape == res['bcv'].shape == (M_,)
    # 1. columns
    rows = res['columns'][:N * Q].reshape(N, Q, C_, S)
    pred = eng.predict(_t(theta), _t(X)).cpu().numpy()                       # [C, S, N, O]
    if task == 'regr':
        assert np.array_equal(rows[:, :O_], np.transpose(pred, (2, 3, 0, 1)), equal_nan=True), (tag, 'mu / log sigma are predict\'s floats')
    ref = np.transpose(ref_cols, (2, 0, 1))
    got = res['columns'].astype(np.float64)
    fin = np.isfinite(ref)
    assert (np.isnan(got) == np.isnan(ref)).all(), (tag, 'NaN pattern of the columns')
    err_c = float(np.abs(got[:N * Q] - ref[:N * Q])[fin[:N * Q]].max())
    scale_c = max(1.0, float(np.abs(ref[:N * Q][fin[:N * Q]]).max()))
    line = f'FDIAG {tag}: columns err {err_c:.3e} bound {1e-4 * scale_c:.3e}'
    if y is not None:
        ll = ref[:N * Q].reshape(N, Q, C_, S)[:, O_]
        scale_l = N * max(1.0, float(np.abs(ll[np.isfinite(ll)]).max()))
        fl = np.isfinite(ref_L)
        err_l = float(np.abs(res['loglik_sum'] - ref_L)[fl].max())
        err_lc = float(np.abs(got[-1] - ref_L)[fl].max())
        line += f'  loglik_sum err {err_l:.3e} (fp32 column {err_lc:.3e}) bound {1e-4 * scale_l:.3e}'
        assert (np.isnan(res['loglik_sum']) == np.isnan(ref_L)).all()
        assert np.array_equal(res['columns'][-1], res['loglik_sum'].astype(np.float32), equal_nan=True)
    else:
        assert res['loglik_sum'] is None
    # 2. statistics: the same kernels on the same floats
    want, path = _chain_diag(raw['columns'], ns)
    assert path == 'library'
    for k in FIVE:
        assert np.array_equal(res[k], want[k], equal_nan=True), (tag, k)
    # 3. summaries
    s, chain = F.summaries(res['rhat'], res['crhat'], res['ess'], N * Q)
    for k in F.SUMMARY:
        g = res['summary'][k]
        if k.endswith(('_mean',)):
            assert (np.isnan(g) and np.isnan(s[k])) or abs(g - s[k]) <= 1e-12 * abs(s[k]), (tag, k, g, s[k])
        else:
            assert (np.isnan(g) and np.isnan(s[k])) or g == s[k], (tag, k, g, s[k])
    assert np.array_equal(res['chain_summary'], chain, equal_nan=True), tag
    line += f'  rhat max {res["summary"]["rhat_max"]:.4f} ess min {res["summary"]["ess_min"]:.1f}'
    print(line)
    assert err_c < 1e-4 * scale_c, (tag, err_c)
    if y is not None:
        assert err_l < 1e-4 * scale_l and err_lc < 1e-4 * scale_l, (tag, err_l, err_lc)
    return res


# case a: M = 16 < one 32-column tile, S at 2 x n_splits x 2; c: the width-64 forward, N past one 32-row pad
FCN_CASES = [('a', 'mfma_narrow_f32', 3, (8, 8, 2), 'tanh', 'regr', 3, 8, 5, 2),
             ('c', 'mfma_w64', 5, (64, 64, 2), 'relu', 'regr', 2, 12, 33, 2),
             ('d', 'auto', 4, (6, 3), 'sigmoid', 'classification', 2, 12, 9, 4)]


@pytest.mark.parametrize('name,kernel,F_,hs,act,task,C_,S,N,ns', FCN_CASES, ids=[c[0] for c in FCN_CASES])
def test_fcn_cases(name, kernel, F_, hs, act, task, C_, S, N, ns):
    ospec, prob, theta, X, y, cols, L, _ = _fcn_case(F_, hs, act, task, C_, S, N, theta_scale=0.05 if hs[0] == 64 else 0.3)
    eng = _fcn_engine(ospec, prob, kernel)
    res = _check(f'{name} {hs} {task} C {C_} S {S} N {N}', eng, theta, X, y, task, cols, L, ns)
    if task != 'regr':                                      # Q = 4, M = 37: the probabilities of a row sum to 1 within 4 ulp
        K = hs[-1]
        p = res['columns'][:N * (K + 1)].reshape(N, K + 1, C_, S)[:, :K].astype(np.float64)
        off = float(np.abs(p.sum(axis=1) - 1.0).max())
        print(f'FDIAG {name}: max |sum_k p_k - 1| = {off:.3e} ({off / np.finfo(np.float32).eps:.2f} ulp)')
        assert res['M'] == 37 and off <= 4 * np.finfo(np.float32).eps


def test_outputs_do_not_depend_on_tiles_or_passes():
    """Case b: 37 rows in tiles of 37, 16 + 16 + 5 and 1, 192 draws in one pass and in passes of 7: every output bit for bit."""
    ospec, prob, theta, X, y, cols, L, _ = _fcn_case(3, (8, 8, 2), 'tanh', 'regr', 3, 64, 37)
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    base = _check('b (3, 64, 37) tiles 0 passes 0', eng, theta, X, y, 'regr', cols, L, 2)
    for rows in (0, 16, 1):
        for draws in (0, 7):
            if (rows, draws) == (0, 0):
                continue
            got = _np(eng.function_diagnostics(_t(theta), _t(X), _t(y), return_columns=True, max_rows_per_tile=rows,
                                               max_draws_per_pass=draws))
            for k in FIVE + ('columns', 'loglik_sum', 'chain_summary'):
                assert np.array_equal(got[k], base[k], equal_nan=True), (rows, draws, k)
            assert got['summary'] == base['summary'], (rows, draws)


def test_lenetti_goes_through_the_same_driver():
    """Case e: a model that is no FCN."""
    from mile_amd import LeNettiSpec
    from mile_amd.engine import Engine
    C_, S, N = 2, 8, 4
    ospec = RL.LeNettiSpec(1, 3, 4, 2, activation='tanh', task='classification')
    prob = RL.synthetic_problem(ospec, 12, C_ * S, seed=6)
    test = RL.synthetic_problem(ospec, N, 1, seed=7)
    eng = Engine(LeNettiSpec(1, 3, 4, 2, activation='tanh', task='classification'), torch.from_numpy(prob['X']),
                 torch.from_numpy(prob['y']), device=DEV)
    assert eng.grad_kernel == 'lenetti_f32'
    out = RL.forward(ospec, prob['theta0'].astype(np.float64), test['X']).reshape(C_, S, N, 2)
    cols, L = F.columns(out, test['y'], 'classification')
    _check('e lenetti C 2 S 8 N 4', eng, prob['theta0'].reshape(C_, S, -1), test['X'].reshape(N, -1), test['y'], 'classification', cols, L, 2)


def test_without_labels_there_is_no_loglik():
    """Case f: Q = O, no L column, no loglik_sum -- and the library refuses one."""
    ospec, prob, theta, X, y, _, _, cols_x = _fcn_case(3, (8, 8, 2), 'tanh', 'regr', 3, 8, 5)
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    res = _check('f (3, 8, 5) no y', eng, theta, X, None, 'regr', cols_x, None, 2)
    assert res['M'] == 10 and res['Q'] == 2
    th, Xd = _t(theta).to(DEV).reshape(-1, theta.shape[2]), _t(X).to(DEV)
    wcv, ls = torch.full((10,), -7.0, device=DEV), torch.full((3, 8), -7.0, dtype=torch.float64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = eng.lib.mile_function_diagnostics(eng._h, p(th), 3, 8, p(Xd), None, 5, 2, 1, p(wcv), None, None, None, None, None, p(ls), None, None,
                                           0, 0, None)
    assert rc == -1 and b'loglik_sum needs y' in eng.lib.mile_last_error()
    torch.cuda.synchronize()
    assert bool((wcv == -7.0).all()) and bool((ls == -7.0).all())


def test_the_pooled_bound_and_past_it():
    """Case g: pooled n = 16 384 exactly runs in the library; 17 500 is refused for ess / rhat with "unsupported" while wcv, bcv,
    crhat and the columns run, and metrics.function_diagnostics returns all five through the torch sort."""
    from mile_amd import _lib
    from mile_amd import metrics as M
    ospec, prob, theta, X, y, cols, L, _ = _fcn_case(3, (8, 8, 2), 'tanh', 'regr', 4, 4096, 1)
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    _check('g (4, 4096, 1)', eng, theta, X, y, 'regr', cols, L, 2)
    ospec, prob, theta, X, y, cols, L, _ = _fcn_case(3, (8, 8, 2), 'tanh', 'regr', 5, 3500, 3)
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    X1, y1 = X[:1], y[:1]
    with pytest.raises(_lib.MileHipError, match='unsupported'):
        eng.function_diagnostics(_t(theta), _t(X1), _t(y1))
    part = eng.function_diagnostics(_t(theta), _t(X1), _t(y1), what=('wcv', 'bcv', 'crhat'), return_columns=True)
    assert part['ess'] is None and part['rhat'] is None and part['summary'] is None
    want, path = _chain_diag(part['columns'], 2)
    assert path == 'library+torch_sort'
    for k in ('wcv', 'bcv', 'crhat'):
        assert np.array_equal(part[k].cpu().numpy(), want[k], equal_nan=True), k
    full = _np(M.function_diagnostics(eng, _t(theta), _t(X1), _t(y1), return_columns=True))
    assert M.LAST_FDIAG_PATH == 'library+torch_sort' and full['M'] == 4
    assert np.array_equal(full['columns'], part['columns'].cpu().numpy())
    for k in FIVE:
        assert np.array_equal(full[k], want[k], equal_nan=True), k
    s, chain = F.summaries(full['rhat'], full['crhat'], full['ess'], 3)
    assert all(full['summary'][k] == pytest.approx(s[k], rel=1e-12) for k in F.SUMMARY)
    assert np.allclose(full['chain_summary'], chain, rtol=1e-12)
    # three rows in blocks of 2 + 1: the blocks' log-likelihood sums, added in block order, are the one call's bit for bit HERE,
    # because (l0 + l1) + l2 is also the row order; with a later block of two or more rows the fp64 sums would associate by
    # block and agree to rounding only (metrics.function_diagnostics says so)
    one = _np(eng.function_diagnostics(_t(theta), _t(X), _t(y), what=('wcv', 'bcv', 'crhat'), return_columns=True))
    walk = _np(M.function_diagnostics(eng, _t(theta), _t(X), _t(y), return_columns=True, block_rows=2))
    assert np.array_equal(walk['loglik_sum'], one['loglik_sum']) and np.array_equal(walk['columns'], one['columns'])
    for k in ('wcv', 'bcv', 'crhat'):
        assert np.array_equal(walk[k], one[k], equal_nan=True), k
    want3, _ = _chain_diag(_t(one['columns']).to(DEV), 2)
    for k in ('ess', 'rhat'):
        assert np.array_equal(walk[k], want3[k], equal_nan=True), k
    err = float(np.abs(walk['loglik_sum'] - L).max())
    print(f'FDIAG g (5, 3500, 3) blocks of 2: loglik_sum err {err:.3e}  rhat max {walk["summary"]["rhat_max"]:.4f}')


def test_permuted_chains_on_the_device():
    """The permutation case of tests/test_fdiag_host.py on the device: the function-space max rhat stays within 1e-3 of the fp64
    reference's (1.0108; hidden-unit order changes fp32 sums, and ranks move only at near-ties), while the parameter-space max
    rhat of the same draws is above 2 (reference 2.4091)."""
    from mile_amd import ModelSpec
    from mile_amd import metrics as M
    from mile_amd.engine import Engine
    spec = ModelSpec(3, F.PERM_WIDTHS, activation='tanh', task='regr')
    theta, X, y, ospec, cols, fn, par = F.permutation_case(tuple((n, o, tuple(sh)) for n, o, sh in spec.leaves()))
    eng = Engine(spec, _t(X), _t(y), device=DEV)
    th = _t(theta.astype(np.float32))
    res = _np(eng.function_diagnostics(th, _t(X), _t(y)))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        p_rhat = M.chain_diagnostics(th.to(DEV), 2)['rhat'].cpu().numpy()
    got, ref = float(res['rhat'].max()), float(fn['rhat'].max())
    print(f'FDIAG permutation: function rhat max {got:.5f} (fp64 {ref:.5f}, diff {abs(got - ref):.2e})  parameter rhat max '
          f'{p_rhat.max():.4f} (fp64 {par["rhat"].max():.4f})  summary {res["summary"]["rhat_max"]:.5f} at column {res["summary"]["rhat_column"]:.0f}')
    assert abs(got - ref) < 1e-3
    assert p_rhat.max() > 2.0
    assert res['summary']['rhat_max'] == float(res['rhat'][:-1].max()) and res['summary']['rhat_gt_1_1'] == 0


def test_a_nan_draw():
    """One draw with a NaN parameter: every column has a NaN in chain 1, so the pooled scores of every column are NaN and so are
    rhat and that chain's crhat, as in tests/diag_ref.py; the other chains' crhat stay finite; the summary counts the cells."""
    ospec, prob, theta0, X, y, cols0, L0, _ = _fcn_case(3, (8, 8, 2), 'tanh', 'regr', 3, 8, 5)
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    theta = theta0.copy()
    theta[1, 3, 0] = np.nan
    cols, L = cols0.copy(), L0.copy()
    cols[1, 3, :] = np.nan
    L[1, 3] = np.nan
    res = _check('nan draw (3, 8, 5)', eng, theta, X, y, 'regr', cols, L, 2)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ref = R.chain_diagnostics(cols, 2)
    for k in FIVE:
        assert (np.isnan(res[k]) == np.isnan(ref[k])).all(), k
    assert np.isnan(res['rhat']).all() and np.isnan(res['crhat'][1]).all() and np.isfinite(res['crhat'][[0, 2]]).all()
    assert np.isnan(res['loglik_sum'][1, 3]) and np.isfinite(np.delete(res['loglik_sum'].reshape(-1), 8 + 3)).all()
    s = res['summary']
    assert s['rhat_skipped'] == 15 and s['crhat_skipped'] == 15 and s['crhat_chain'] in (0, 2) and np.isnan(s['rhat_max']) and s['rhat_column'] == -1
    assert s['ess_skipped'] == int((~np.isfinite(res['ess'][:, :15])).sum())


def test_refusals_leave_the_outputs_and_the_handle_alone():
    from mile_amd import _lib
    ospec, prob, theta, X, y, cols, L, _ = _fcn_case(3, (8, 8, 2), 'tanh', 'regr', 3, 8, 5)
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    lib, B = eng.lib, _lib.DIAG_BITS
    every = B['wcv'] | B['bcv'] | B['ess'] | B['crhat'] | B['rhat']
    th, Xd, yd = _t(theta).to(DEV).reshape(24, -1), _t(X).to(DEV), _t(y).to(DEV)
    M_ = 16
    f32 = {k: torch.full((3 * M_,) if k in ('ess', 'crhat') else (M_,), -7.0, device=DEV) for k in FIVE}
    f64 = {k: torch.full((n,), -7.0, dtype=torch.float64, device=DEV) for k, n in (('loglik_sum', 24), ('summary', 16), ('chain_summary', 6))}
    colsd = torch.full((M_ * 24,), -7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(theta_=th, C_=3, S=8, N=5, ns=2, what=every, outs=None, h=None):
        o = dict(f32) if outs is None else outs
        return lib.mile_function_diagnostics(h or eng._h, p(theta_), C_, S, p(Xd), p(yd), N, ns, what, *[p(o.get(k)) for k in FIVE], p(colsd),
                                             p(f64['loglik_sum']), p(f64['summary']), p(f64['chain_summary']), 0, 0, None)

    def refused(rc, word):
        msg = lib.mile_last_error()
        assert rc == -1 and b'mile_function_diagnostics: ' in msg and word in msg, (rc, msg)

    refused(call(theta_=None), b'null argument')
    refused(call(ns=3), b'n_splits must divide S')
    refused(call(S=2), b'4 <= S <= 4096')
    refused(call(what=every | B['pooled_input']), b'MILE_DIAG_POOLED_INPUT')
    refused(call(what=B['wcv']), b'not in `what`')                             # the other four pointers are still there
    refused(call(what=every, outs={k: f32[k] for k in ('wcv', 'bcv', 'ess', 'crhat')}), b'null pointer for an output asked for')
    refused(call(what=B['wcv'] | B['bcv'] | B['crhat'], outs={k: f32[k] for k in ('wcv', 'bcv', 'crhat')}), b'summary and chain_summary need')
    for bad in ((0, 8, 5), (3, 2, 5), (3, 4097, 5), (3, 8, 0), (70000, 8, 5)):
        assert lib.mile_function_diagnostics_workspace(eng._h, *bad, 1) == -1, bad
    assert lib.mile_function_diagnostics_workspace(eng._h, 3, 8, 5, 1) > lib.mile_function_diagnostics_workspace(eng._h, 3, 8, 5, 0) > 0
    # more than 64 head outputs: the argument logic alone, no such net is run
    wide = O.ModelSpec(3, (4, 65), activation='tanh', task='classification')
    wprob = O.synthetic_problem(wide, 8, 1, seed=1)
    weng = _fcn_engine(wide, wprob)
    wth = torch.zeros((24, weng.d), device=DEV)
    refused(call(theta_=wth, h=weng._h), b'more than 64 head outputs')
    assert lib.mile_function_diagnostics_workspace(weng._h, 3, 8, 5, 1) == -1
    torch.cuda.synchronize()
    for t in (*f32.values(), *f64.values(), colsd):
        assert bool((t == -7.0).all())
    assert call() == 0, lib.mile_last_error()                                 # the same call, valid, on the same handle
    torch.cuda.synchronize()
    for t in (*f32.values(), *f64.values(), colsd):
        assert not bool((t == -7.0).any())
    res = _np(eng.function_diagnostics(_t(theta), _t(X), _t(y), return_columns=True))
    assert np.array_equal(f32['rhat'].cpu().numpy(), res['rhat']) and np.array_equal(colsd.cpu().numpy().reshape(M_, 3, 8), res['columns'])
    assert np.array_equal(f64['loglik_sum'].cpu().numpy().reshape(3, 8), res['loglik_sum'])


def test_evaluate_cli_function_diagnostics(tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=80, n_chains=4)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, str(ROOT / 'train.py'), '-c', str(tmp_path / 'cfg.yaml'), '-d', '1'],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp = tmp_path / 'smoke_synthetic'
    r = subprocess.run([sys.executable, str(ROOT / 'evaluate.py'), '-e', str(exp), '--function-diagnostics'], capture_output=True,
                       text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = json.loads((exp / 'metrics.json').read_text())
    C_, S, N = m['n_chains'], m['n_samples'], m['n_points']
    z = np.load(exp / 'function_diagnostics.npz')
    Q = int(z['Q'])
    M_ = N * Q + 1
    assert z['ess'].shape == z['crhat'].shape == (C_, M_) and z['rhat'].shape == z['wcv'].shape == z['bcv'].shape == (M_,)
    assert z['loglik_sum'].shape == (C_, S) and z['chain_summary'].shape == (C_, 2) and m['fdiag_n_columns'] == M_
    assert all(np.isfinite(z[k]).all() for k in ('ess', 'crhat', 'rhat', 'wcv', 'bcv', 'loglik_sum', 'chain_summary'))
    assert m['fdiag_n_splits'] == 2 and m['fdiag_rhat_max'] == float(z['rhat'][:-1].max())
    assert m['fdiag_ess_min'] == float(z['ess'][:, :-1].min()) and m['fdiag_loglik_sum_rhat'] == float(z['rhat'][-1])
    assert 0.0 < m['fdiag_r_eff_mean'] and 0.0 <= m['fdiag_between_share'] <= 1.0 and len(m['fdiag_chain_ess_min']) == C_
    r = subprocess.run([sys.executable, str(ROOT / 'evaluate.py'), '-e', str(exp)], capture_output=True, text=True, cwd=ROOT,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert not any(k.startswith('fdiag_') for k in json.loads((exp / 'metrics.json').read_text()))
