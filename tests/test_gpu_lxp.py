"""mile_psis_expect / mile_loo_predict_stream (Engine.psis_expect, Engine.loo_predict_stream) against the fp64 restatement of
tests/lxp_ref.py (-m gpu): the kernels on crafted log-likelihoods in every regime of tests/test_gpu_loo.py, the tie rule, the
streamed call bit for bit under every pass and tile size and against the restatement fed with the library's own tensors, end to
end through the forward kernels, the refusals, and evaluate.py --loo-predict.

Bounds.  On a given fp32 tensor every output is within 1e-9 max(1, |value|) of the restatement of the same tensor, the project's
bound for "the new kernels alone" (tests/test_gpu_loo.py), with equal NaN patterns and equal ``dropped``; sums that are 1 by
construction (a row of weights, the expectation of the constant column) to 1e-12: S <= 2^20 terms in fp64, the runs of a row
combined in a fixed order.  khat and elpd_loo are the operations of mile_psis_loo in its order: 1e-12 max(1, |value|).  End to
end the device forward is fp32 and no output is 1-Lipschitz in it, so the bound is measured from the reference alone, by the
method of tests/test_gpu_loo.py: the largest change of the restatement's output over four seeded perturbations of its fp64
inputs, each uniform within +- the measured forward error (of the log-likelihoods and of the raw outputs), times 8, + 1e-9 --
asserted on the rows whose reference khat is at most 0.7, which must be at least 80 % of a case's rows.

Measured on an MI355X: see DESIGN.md section 3.2x."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import loo_ref as LR
from tests import lxp_ref as XR
from tests.test_gpu_loo import FCN, SEVEN, _engine, _fcn_case, _np, _tensor
from tests.test_gpu_predict import DEV, ROOT, _fcn_engine, _run
from tests.test_lxp_host import _values, check_against_ref

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ALL = ('expect', 'posterior', 'ess_w', 'khat', 'elpd_loo', 'dropped', 'weights')
ROWS = ('expect', 'posterior', 'ess_w', 'khat', 'elpd_loo')


# ---- a. the kernels on given tensors ---------------------------------------------------------------------------------------
def _check_given(tag, ll, v, r_eff=1.0):
    eng = _engine()
    got = _np(eng.psis_expect(torch.from_numpy(ll), torch.from_numpy(v), r_eff=r_eff, outputs=ALL))
    ref = XR.expect(ll, v, r_eff)
    assert got['dropped'].dtype == np.int32 and all(got[k].dtype == np.float64 for k in ALL if k != 'dropped')
    check_against_ref(tag, got, ref)
    w = got['weights']
    ok = ~np.isnan(w).any(axis=1)
    assert np.abs(w[ok].sum(axis=1) - 1.0).max(initial=0.0) <= 1e-12, (tag, w[ok].sum(axis=1))
    assert (w[~np.isfinite(ll.T)][~np.isnan(w[~np.isfinite(ll.T)])] == 0.0).all(), tag      # a dropped draw: exactly 0
    for n in np.nonzero(ok)[0]:                                                            # equal l bits, equal weight bits
        keep = np.isfinite(ll[:, n])
        _, first, inv = np.unique(ll[keep, n].view(np.uint32), return_index=True, return_inverse=True)
        assert (w[n, keep].view(np.uint64) == w[n, keep][first][inv.reshape(-1)].view(np.uint64)).all(), (tag, n)
    loo = _np(eng.psis_loo(torch.from_numpy(ll), r_eff=r_eff))
    for k in ('khat', 'elpd_loo'):
        assert (np.isnan(got[k]) == np.isnan(loo[k])).all(), (tag, k)
        fin = ~np.isnan(loo[k])
        assert (np.abs(got[k][fin] - loo[k][fin]) <= 1e-12 * np.maximum(1.0, np.abs(loo[k][fin]))).all(), (tag, k, got[k], loo[k])
    return got, ref


@pytest.mark.parametrize('S', [2, 20, 21, 26, 70, 1000, 16384, 16385])
def test_every_regime_on_given_tensors(S):
    """S = 2: the smallest call; 20 / 21: M = 4 (no fit) and M = 5 (the smallest fit); 16 384 / 16 385: the row in LDS and
    streamed from the packed copy.  Columns: standard normal, l itself, the constant 1."""
    ll = _tensor(S, SEVEN, 100 + S)
    got, ref = _check_given(f'S={S}', ll, _values(ll, S))
    assert np.abs(got['expect'][:, 2] - 1.0).max() <= 1e-12 and (got['posterior'][:, 2] == 1.0).all()
    assert np.abs(got['weights'][4] - 1.0 / S).max() <= 1e-15 and abs(got['ess_w'][4] - S) <= 1e-9 * S      # the constant row
    if S >= 20:
        assert ref['dropped'].tolist() == [0] * 6 + [3]
    if S >= 1000:
        lv = ll[:, 5]                                              # 'eight-levels': the lowest level alone is longer than the tail
        assert (lv == lv.min()).sum() > LR.tail_length(S)


def test_ties_across_the_tail_boundary_do_not_see_the_order_of_the_draws():
    """40 levels of about 5 copies, M = 40: the cut level has copies in the tail and in the body, runs of equal keys fill the tail,
    and the values are distinct.  Permuting the draws moves expect by the rounding of a sum in another order."""
    S = 200
    rng = np.random.default_rng(12)
    l = (-0.25 * np.floor(40.0 * rng.uniform(size=S)) - 0.3).astype(np.float32)
    srt = np.sort(l)
    M = LR.tail_length(S)
    assert srt[M - 1] == srt[M] and M == 40                        # the (M+1)-th smallest equals the M-th: a tie across the boundary
    ll = np.ascontiguousarray(np.stack([l, l[::-1]], axis=1))
    v = rng.standard_normal((S, 2, 1)).astype(np.float32)
    v[:, 1] = v[::-1, 0]                                           # row 1 is row 0 with the draws reversed
    got, _ = _check_given('boundary ties', ll, v)
    perm = rng.permutation(S)
    moved = _np(_engine().psis_expect(torch.from_numpy(np.ascontiguousarray(ll[perm])), torch.from_numpy(np.ascontiguousarray(v[perm])),
                                      outputs=('expect', 'weights')))
    print('boundary ties: max |expect - expect of permuted draws| =', np.abs(moved['expect'] - got['expect']).max(),
          '; rows 0 and 1 (reversed):', abs(got['expect'][0, 0] - got['expect'][1, 0]))
    assert np.abs(moved['expect'] - got['expect']).max() <= 1e-12 and abs(got['expect'][0, 0] - got['expect'][1, 0]) <= 1e-12
    assert np.abs(moved['weights'] - got['weights'][:, perm]).max() <= 1e-15       # a draw's weight is a function of the multiset


def test_rows_with_fewer_than_two_finite_draws():
    ll = _tensor(26, ('light', 'light', 'heavy0.6', 'light'), 7)
    ll[:, 1] = np.nan                                              # nothing kept
    ll[1:, 3] = np.inf                                             # one draw kept
    got, _ = _check_given('too few', ll, _values(ll, 3))
    assert got['dropped'].tolist() == [0, 26, 0, 25]
    assert all(np.isnan(got[k][[1, 3]]).all() and np.isfinite(got[k][[0, 2]]).all() for k in ('expect', 'posterior', 'ess_w', 'elpd_loo', 'weights'))


@pytest.mark.parametrize('S', [116508, 116509, 1 << 20])
def test_the_sort_s_padding_boundary_and_the_longest_tail(S):
    """M = 1024 and 1025: a tail that fills its power of two and one that starts the next; S = 2^20: M = 3072.  One row, Q = 1."""
    assert LR.tail_length(S) == {116508: 1024, 116509: 1025, 1 << 20: 3072}[S]
    ll = _tensor(S, ('heavy1.5',), S % 1000)
    _check_given(f'S={S}', ll, np.random.default_rng(S).standard_normal((S, 1, 1)).astype(np.float32))


def test_outputs_are_optional_one_by_one():
    ll = _tensor(70, SEVEN, 5)
    v = _values(ll, 6)
    eng = _engine()
    full = _np(eng.psis_expect(torch.from_numpy(ll), torch.from_numpy(v), outputs=ALL))
    for k in ALL:
        only = _np(eng.psis_expect(torch.from_numpy(ll), torch.from_numpy(v), outputs=(k,)))
        assert list(only) == [k] and only[k].tobytes() == full[k].tobytes(), k
    bare = _np(eng.psis_expect(torch.from_numpy(ll)))              # no values: everything but the sums
    assert sorted(bare) == ['dropped', 'elpd_loo', 'ess_w', 'khat'] and all(bare[k].tobytes() == full[k].tobytes() for k in bare)


# ---- b. the streamed call ---------------------------------------------------------------------------------------------------
STREAM = {
    # F, hidden_structure, activation, task, kernel
    'narrow-regr': (5, (16, 16, 2), 'relu', 'regr', 'mfma_narrow_f32'),
    'generic-class': (6, (8, 4), 'tanh', 'classification', 'generic'),
}
N_ST, C_ST, S_ST = 70, 2, 35


@functools.lru_cache(maxsize=None)
def _stream_case(name):
    F, hs, act, task, _ = STREAM[name]
    ospec = O.ModelSpec(F, hs, activation=act, task=task)
    prob = O.synthetic_problem(ospec, 64, 1, seed=3, theta_scale=0.3)
    test = O.synthetic_problem(ospec, N_ST, 1, seed=4)
    base = prob['theta0'][0].astype(np.float64)
    theta = (base[None, None] + 0.05 * np.random.default_rng(5).standard_normal((C_ST, S_ST, base.shape[0]))).astype(np.float32)
    return ospec, prob, theta, np.ascontiguousarray(test['X']), np.ascontiguousarray(test['y'])


@pytest.mark.parametrize('name', list(STREAM))
def test_stream_for_every_pass_and_tile_and_against_the_library_s_own_tensors(name):
    ospec, prob, theta, X, y = _stream_case(name)
    eng = _fcn_engine(ospec, prob, STREAM[name][4])
    th, Xt, yt = torch.from_numpy(theta), torch.from_numpy(X), torch.from_numpy(y)
    base = _np(eng.loo_predict_stream(th, Xt, yt))
    Q = 4 if ospec.task == 'regr' else ospec.hidden_structure[-1]
    assert base['expect'].shape == (N_ST, Q) and np.isfinite(base['expect']).all() and not base['dropped'].any()
    for draws in (0, 7, 70):
        for rows in (0, 32, 64):                                   # 32 at N = 70: two full tiles and a ragged one of 6
            got = _np(eng.loo_predict_stream(th, Xt, yt, max_draws_per_pass=draws, max_rows_per_tile=rows))
            for k in base:
                assert got[k].tobytes() == base[k].tobytes(), (name, draws, rows, k)
    loo = _np(eng.loo_stream(th, Xt, yt))
    for k in ('khat', 'elpd_loo'):
        assert (np.isnan(base[k]) == np.isnan(loo[k])).all()
        fin = ~np.isnan(loo[k])
        assert (np.abs(base[k][fin] - loo[k][fin]) <= 1e-12 * np.maximum(1.0, np.abs(loo[k][fin]))).all(), (name, k)
    ll = eng.pointwise_loglik(th, Xt, yt).reshape(-1, N_ST).cpu().numpy()
    raw = eng.predict(th, Xt).reshape(C_ST * S_ST, N_ST, -1).cpu().numpy()
    ref = XR.expect(ll, XR.columns(raw, y, ospec.task))
    check_against_ref(f'stream {name}', base, ref, keys=('expect', 'posterior', 'ess_w'))
    if ospec.task == 'regr':
        assert ((base['expect'][:, 3] >= 0.0) & (base['expect'][:, 3] <= 1.0 + 1e-12)).all()      # (sum w = 1 up to rounding)
    else:
        assert np.abs(base['expect'].sum(axis=1) - 1.0).max() <= 1e-12
    # one workspace for every streamed call of the handle: another call in between changes nothing
    eng.predict_moments(th.reshape(-1, th.shape[-1]), Xt)
    again = _np(eng.loo_predict_stream(th, Xt, yt))
    assert all(again[k].tobytes() == base[k].tobytes() for k in base)


# ---- c. end to end against the fp64 forward ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(FCN))
def test_stream_end_to_end_against_the_fp64_forward(name):
    ospec, prob, theta, X, y = _fcn_case(name)
    eng = _fcn_engine(ospec, prob, FCN[name][4])
    out64 = O.mlp_forward(ospec, theta.astype(np.float64), X.astype(np.float64))             # [S, N, O]
    pw64 = O.pointwise_lppd(ospec, out64[None], y)[0]                                        # [S, N]
    th, Xt, yt = torch.from_numpy(theta), torch.from_numpy(X), torch.from_numpy(y)
    err_l = float(np.abs(eng.pointwise_loglik(th, Xt, yt).cpu().numpy().astype(np.float64) - pw64).max())
    err_z = float(np.abs(eng.predict(th, Xt).cpu().numpy().astype(np.float64) - out64).max())
    ref = XR.expect(pw64, XR.columns(out64, y, ospec.task))
    held = ref['khat'] <= 0.7                                      # (NaN: not held)
    share = float(held.mean())
    change = {k: 0.0 for k in ROWS}
    for seed in range(4):
        rng = np.random.default_rng(100 + seed)
        moved = XR.expect(pw64 + rng.uniform(-err_l, err_l, pw64.shape), XR.columns(out64 + rng.uniform(-err_z, err_z, out64.shape), y, ospec.task))
        for k in ROWS:
            change[k] = max(change[k], float(np.abs(moved[k] - ref[k])[held].max()))
    bound = {k: 8.0 * change[k] + 1e-9 for k in ROWS}
    got = _np(eng.loo_predict_stream(th, Xt, yt))
    dev = {k: float(np.abs(got[k] - ref[k])[held].max()) for k in ROWS}
    print(f'{name}: max|pointwise_loglik - fp64| = {err_l:.3e}, max|predict - fp64| = {err_z:.3e}; rows with khat <= 0.7: {100 * share:.1f} %')
    print(f'{name}: device error | bound (worst ratio {max(dev[k] / bound[k] for k in ROWS):.3f}): '
          + ', '.join(f'{k} {dev[k]:.3e} | {bound[k]:.3e}' for k in ROWS))
    assert share >= 0.8, (name, share)
    assert not got['dropped'].any() and (np.isnan(got['khat']) == np.isnan(ref['khat'])).all()
    for k in ROWS:
        assert dev[k] <= bound[k], (name, k, dev[k], bound[k])


# ---- d. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_and_the_handle_alone():
    from mile_amd import _lib
    ospec, prob, theta, X, y = _stream_case('narrow-regr')
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    th, Xt, yt = torch.from_numpy(theta).to(DEV).reshape(-1, theta.shape[-1]), torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)
    ll = eng.pointwise_loglik(th, Xt, yt)
    v = torch.ones((ll.shape[0], ll.shape[1], 2), device=DEV)
    before = _np(eng.loo_predict_stream(th, Xt, yt))
    for tag, fn in [('S = 1, psis_expect', lambda: eng.psis_expect(ll[:1], v[:1])), ('S = 1, stream', lambda: eng.loo_predict_stream(th[:1], Xt, yt)),
                    ('r_eff = 0, psis_expect', lambda: eng.psis_expect(ll, v, r_eff=0.0)),
                    ('r_eff NaN, stream', lambda: eng.loo_predict_stream(th, Xt, yt, r_eff=float('nan'))),
                    ('Q = 65', lambda: eng.psis_expect(ll, torch.ones((ll.shape[0], ll.shape[1], 65), device=DEV))),
                    ('tile < 0', lambda: eng.loo_predict_stream(th, Xt, yt, max_rows_per_tile=-1))]:
        with pytest.raises(_lib.MileHipError, match='libmile_hip error -1') as exc:
            fn()
        print(tag, '->', exc.value)
    p = lambda t: C.c_void_p(t.data_ptr())
    S, N = ll.shape
    marked = torch.full((N, 2), 7.0, dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.MileHipError, match='libmile_hip error -1: mile_psis_expect: expect and posterior need values'):
        _lib.check(eng.lib.mile_psis_expect(p(ll), None, S, N, 2, 1.0, p(marked), None, None, None, None, None, None, None), eng.lib)
    with pytest.raises(_lib.MileHipError, match='libmile_hip error -1: mile_psis_expect: Q out of range'):
        _lib.check(eng.lib.mile_psis_expect(p(ll), p(v), S, N, 0, 1.0, p(marked), None, None, None, None, None, None, None), eng.lib)
    with pytest.raises(_lib.MileHipError, match='libmile_hip error -1: mile_loo_predict_stream: no output'):
        _lib.check(eng.lib.mile_loo_predict_stream(eng._h, p(th), S, p(Xt), p(yt), N, 1.0, None, None, None, None, None, None, 0, 0, None), eng.lib)
    assert (marked == 7.0).all() and eng.loo_predict_stream_workspace(1, 70) == -1 and eng.loo_predict_stream_workspace(70, 70) > 0
    after = _np(eng.loo_predict_stream(th, Xt, yt))
    assert all(after[k].tobytes() == before[k].tobytes() for k in before)


# ---- e. evaluate.py --loo-predict --------------------------------------------------------------------------------------------
def _train_and_evaluate(tmp_path, cfg, name):
    import yaml
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    _run([ROOT / 'train.py', '-c', tmp_path / 'cfg.yaml', '-d', '1'])
    exp = tmp_path / name
    _run([ROOT / 'evaluate.py', '-e', exp, '--loo'])
    plain = json.loads((exp / 'metrics.json').read_text())
    assert not (exp / 'loo_predict.npz').exists() and not any(k.startswith('loopred_') for k in plain)
    _run([ROOT / 'evaluate.py', '-e', exp, '--loo', '--loo-predict'])
    m = json.loads((exp / 'metrics.json').read_text())
    assert {k: v for k, v in m.items() if not k.startswith('loopred_')} == plain
    return m, np.load(exp / 'loo_predict.npz'), np.load(exp / 'loo.npz')


def test_evaluate_cli_loo_predict_regression(tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=120, n_chains=4)      # thinning 10: 12 draws kept per chain
    m, z, loo = _train_and_evaluate(tmp_path, cfg, 'smoke_synthetic')
    N = loo['khat'].shape[0]
    assert sorted(z.files) == ['dropped', 'ess_w', 'expect', 'khat', 'pit', 'posterior']
    assert z['expect'].shape == z['posterior'].shape == (N, 4) and all(z[k].shape == (N,) for k in ('dropped', 'ess_w', 'khat', 'pit'))
    assert ((z['pit'] >= 0.0) & (z['pit'] <= 1.0)).all() and np.abs(z['pit'] - z['expect'][:, 3]).max() <= 1e-12
    assert z['khat'].tobytes() == loo['khat'].tobytes() and m['loopred_n_rows'] == N and m['split'] == 'test'
    for k in ('rmse', 'r2', 'var_epistemic', 'var_aleatoric', 'cal_error', 'coverage_0.5', 'coverage_0.95'):
        assert np.isfinite(m['loopred_' + k]) and np.isfinite(m['loopred_' + k + '_insample']), k
    for k in ('khat_above_0.7_share', 'ess_w_min', 'ess_w_median', 'dropped'):
        assert 'loopred_' + k in m, k
    print(f"cli regression: rmse {m['loopred_rmse']:.4f} (in-sample {m['loopred_rmse_insample']:.4f}), cal_error {m['loopred_cal_error']:.4f} "
          f"(in-sample {m['loopred_cal_error_insample']:.4f}), min ess_w {m['loopred_ess_w_min']:.1f}")
    assert 1.0 <= m['loopred_ess_w_min'] <= 48.0 + 1e-9 and (z['expect'][:, 2] > 0.0).all()


def test_evaluate_cli_loo_predict_classification(tmp_path):
    import yaml
    rng = np.random.default_rng(5)
    N, F, K = 240, 6, 3
    X = rng.standard_normal((N, F))
    labels = np.argmax(1.5 * X @ rng.standard_normal((F, K)) + rng.gumbel(size=(N, K)), axis=1)
    np.save(tmp_path / 'three.npy', np.concatenate([X, labels[:, None]], axis=1).astype(np.float32))
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['experiment_name'] = 'three_classes'
    cfg['data'].update(path=str(tmp_path / 'three.npy'), source='local', task='class')
    cfg['model']['hidden_structure'] = [16, 16, K]
    cfg['training']['sampler'].update(warmup_steps=40, n_samples=60, n_chains=2)       # thinning 10: 6 draws kept per chain
    m, z, loo = _train_and_evaluate(tmp_path, cfg, 'three_classes')
    Nt = loo['khat'].shape[0]
    assert sorted(z.files) == ['dropped', 'ess_w', 'expect', 'khat', 'posterior'] and z['expect'].shape == (Nt, K)
    assert np.abs(z['expect'].sum(axis=1) - 1.0).max() <= 1e-12 and z['khat'].tobytes() == loo['khat'].tobytes()
    assert abs(m['loopred_nll'] + loo['elpd_loo'].mean()) <= 1e-9
    for k in ('accuracy', 'brier', 'nll', 'ece', 'mce'):
        assert np.isfinite(m['loopred_' + k]) and np.isfinite(m['loopred_' + k + '_insample']), k
    print(f"cli classification: accuracy {m['loopred_accuracy']:.3f} (in-sample {m['loopred_accuracy_insample']:.3f}), "
          f"nll {m['loopred_nll']:.4f} (in-sample {m['loopred_nll_insample']:.4f})")
