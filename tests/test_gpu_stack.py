"""mile_stack_eval and mile_chain_loo_stream (Engine.stack_eval, Engine.chain_loo_stream) on the device (-m gpu): the stacking
evaluation against the fp64 restatement of tests/stack_ref.py over every tile and block path, bit for bit under every tile
size, the per-chain PSIS-LOO against mile_loo_stream of each chain's slice, the solver on the kernels, the refusals, and
evaluate.py --stacking.

Bounds.  Every output of mile_stack_eval is within 1e-9 max(1, |value|) of the restatement, entry by entry -- the bound
tests/test_gpu_loo.py uses for the same kind of fixed-order fp64 sums -- with equal NaN patterns and equal ``used``.

Shapes.  C = 1: the two extra rows alone; 17: a ragged 4 x 4 register block; 62 / 63 / 64 / 65: the rows C and C + 1 inside one
64-chain tile, split over two, and alone in the second; 128: three tiles.  N = 1: one row; 63 / 64 / 65: around two blocks of 32
and the 16-row LDS step; 1052: 33 blocks.  1024 x 300: the largest C, 17 tile rows, 5 blocks of 64.

Measured on an MI355X: see DESIGN.md section 3.2r."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

from mile_amd import metrics as M
from oracle import mclmc_oracle as O
from tests import stack_ref as SR
from tests.test_gpu_predict import DEV, ROOT, _fcn_engine, _reload, _run

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

OUT = ('score', 'row_score', 'grad', 'hess', 'used')
_ENGINE = {}


def _engine():
    """Any engine: mile_stack_eval needs no handle, only the library and the device."""
    if 'e' not in _ENGINE:
        ospec = O.ModelSpec(5, (16, 16, 2), activation='relu', task='regr')
        _ENGINE['e'] = _fcn_engine(ospec, O.synthetic_problem(ospec, 64, 1, seed=3, theta_scale=0.3), 'mfma_narrow_f32')
    return _ENGINE['e']


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def _case(Cn, N):
    """The distinct family with the rows the definition leaves out: a NaN, a +inf and a row of -inf; and one -inf that stays."""
    lpd = SR.make_case('distinct', Cn, N).copy()
    if N >= 7:
        lpd[Cn // 2, 1] = np.nan
        lpd[:, 3] = -np.inf
        lpd[Cn - 1, 4] = np.inf
        if Cn > 1:
            lpd[0, 5] = -np.inf
    return lpd


def _weights(Cn):
    zeros = np.where(np.arange(Cn) % 3 == 1, 0.0, 1.0)
    zeros[Cn - 1] = 1.0
    hot = np.zeros(Cn)
    hot[Cn - 1] = 1.0
    return {'uniform': np.full(Cn, 1.0 / Cn), 'zeros': zeros / zeros.sum(), 'one-hot': hot}


def _check(tag, lpd, w, tile=0):
    got = _np(_engine().stack_eval(torch.from_numpy(lpd), torch.from_numpy(w), outputs=OUT, max_rows_per_tile=tile))
    ref = SR.stack_eval_ref(lpd, w)
    assert int(got['used']) == ref['used'] and got['used'].dtype == np.int64, (tag, got['used'], ref['used'])
    worst = {}
    for k in ('score', 'row_score', 'grad', 'hess'):
        g, r = got[k], np.asarray(ref[k], dtype=np.float64)
        assert g.dtype == np.float64 and g.shape == r.shape, (tag, k, g.shape, r.shape)
        assert (np.isnan(g) == np.isnan(r)).all(), (tag, k, 'NaN pattern')
        fin = ~np.isnan(r)
        with np.errstate(invalid='ignore'):
            rel = np.abs(g[fin] - r[fin]) / np.maximum(1.0, np.abs(r[fin]))
        rel = np.where(g[fin] == r[fin], 0.0, rel)                         # (-inf against -inf)
        worst[k] = float(rel.max()) if fin.any() else 0.0
    print(f'{tag}: used {ref["used"]}, max |out - ref| / max(1, |ref|) = ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1e-9, (tag, k, v)
    assert np.array_equal(got['hess'], got['hess'].T), tag
    return got, ref


# ---- a. the evaluation against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize('Cn', [1, 3, 12, 17, 64, 65, 128])
def test_stack_eval_is_the_definition(Cn):
    for N in (1, 7, 63, 64, 65, 1052):
        lpd = _case(Cn, N)
        for name, w in _weights(Cn).items():
            got, ref = _check(f'{Cn} x {N}, {name}', lpd, w)
            if N >= 7:
                assert ref['used'] == N - 3 and np.isnan(got['row_score'][[1, 3, 4]]).all() and np.isfinite(got['row_score'][5])


@pytest.mark.parametrize('Cn', [62, 63])
def test_the_two_extra_rows_across_a_tile_of_chains(Cn):
    for name, w in _weights(Cn).items():
        _check(f'{Cn} x 65, {name}', _case(Cn, 65), w)


def test_stack_eval_at_the_largest_c():
    lpd = _case(1024, 300)
    for name, w in _weights(1024).items():
        _check(f'1024 x 300, {name}', lpd, w)


def test_a_used_row_without_mass_makes_the_score_minus_inf():
    lpd = SR.make_case('distinct', 3, 7).copy()
    lpd[1:, 2] = -np.inf
    w = np.array([0.0, 0.5, 0.5])
    got = _np(_engine().stack_eval(torch.from_numpy(lpd), torch.from_numpy(w), outputs=('score', 'row_score', 'used')))
    assert got['score'] == -np.inf and int(got['used']) == 7 and got['row_score'][2] == -np.inf
    assert np.isfinite(np.delete(got['row_score'], 2)).all()
    sol = M.stacking_weights(torch.from_numpy(lpd), eval=_engine().stack_eval, w0=w)
    assert sol['converged'] is False and sol['score'] == -np.inf          # a rejected start, no exception
    none = np.full((3, 7), np.nan)
    got = _np(_engine().stack_eval(torch.from_numpy(none), torch.from_numpy(w), outputs=OUT))
    assert int(got['used']) == 0 and np.isnan(got['score']) and np.isnan(got['grad']).all() and np.isnan(got['row_score']).all()


# ---- b. the same bits for every tile, and for every subset of the outputs -----------------------------------------------
@pytest.mark.parametrize('Cn,N', [(3, 7), (12, 1052), (65, 1052), (128, 65), (1024, 300)])
def test_outputs_do_not_depend_on_the_tile(Cn, N):
    lpd, w = torch.from_numpy(_case(Cn, N)).to(DEV), torch.from_numpy(_weights(Cn)['zeros']).to(DEV)
    eng = _engine()
    base = _np(eng.stack_eval(lpd, w, outputs=OUT))
    for tile in (32, 33, N):
        got = _np(eng.stack_eval(lpd, w, outputs=OUT, max_rows_per_tile=tile))
        for k in OUT:
            assert np.array_equal(got[k], base[k], equal_nan=True) and got[k].tobytes() == base[k].tobytes(), (Cn, N, tile, k)
    for outs in (('score',), ('score', 'grad'), ('grad',), ('used',), ('row_score',), ('hess',)):
        got = _np(eng.stack_eval(lpd, w, outputs=outs, max_rows_per_tile=33))
        for k in outs:
            assert got[k].tobytes() == base[k].tobytes(), (Cn, N, outs, k)


# ---- c. per-chain PSIS-LOO ---------------------------------------------------------------------------------------------------
KEYS = ('lppd', 'p_waic', 'elpd_loo', 'khat', 'dropped')


@pytest.mark.parametrize('name', ['narrow-regr', 'generic-class'])
def test_chain_loo_is_loo_stream_of_each_chain(name):
    from tests.test_gpu_loo import FCN, _fcn_case
    ospec, prob, theta, X, y = _fcn_case(name)
    eng = _fcn_engine(ospec, prob, FCN[name][4])
    Cn, S = 3, 70
    samples = torch.from_numpy(np.ascontiguousarray(theta[:Cn * S].reshape(Cn, S, -1)))
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    assert X.shape[0] == 70
    full = _np(eng.chain_loo_stream(samples, Xt, yt))
    assert all(full[k].shape == (Cn, 70) for k in KEYS) and full['dropped'].dtype == np.int32 and np.isfinite(full['elpd_loo']).all()
    for c in range(Cn):
        alone = _np(eng.loo_stream(samples[c], Xt, yt))
        for k in KEYS:
            assert np.array_equal(full[k][c], alone[k], equal_nan=True) and full[k][c].tobytes() == alone[k].tobytes(), (name, c, k)
    for draws, rows in ((7, 0), (0, 32), (33, 33)):                        # 32 at N = 70: two full tiles and a ragged one
        got = _np(eng.chain_loo_stream(samples, Xt, yt, max_draws_per_pass=draws, max_rows_per_tile=rows))
        for k in KEYS:
            assert got[k].tobytes() == full[k].tobytes(), (name, draws, rows, k)
    only = _np(eng.chain_loo_stream(samples, Xt, yt, outputs=('lppd',)))
    assert sorted(only) == ['lppd'] and only['lppd'].tobytes() == full['lppd'].tobytes()
    assert eng.chain_loo_stream_workspace(Cn, S, 70) == eng.loo_stream_workspace(S, 70)
    # the held-out matrix at equal weights is the ensemble's LPPD of the stream
    stream = float(eng.lppd_stream(samples, Xt, yt, curve_points=[])['lppd'])
    equal = M.weighted_lppd(torch.from_numpy(full['lppd']), np.full(Cn, 1.0 / Cn), eval=eng.stack_eval)
    print(f'{name}: weighted_lppd at 1 / C = {equal!r}, lppd_stream = {stream!r}')
    assert abs(equal - stream) <= 1e-9 * max(1.0, abs(stream))


# ---- d. the solver on the kernels ---------------------------------------------------------------------------------------------
def test_solver_on_the_device_follows_the_reference():
    lpd = SR.make_case('distinct', 12, 1052)
    ref = SR.stacking_weights_ref(lpd)
    assert ref['converged'] and SR.support_condition(lpd, ref['w']) < 1e8
    eng = _engine()
    got = M.stacking_weights(torch.from_numpy(lpd).to(DEV), eval=eng.stack_eval)
    print(f'device solver: {got["iterations"]} Newton steps ({ref["iterations"]}), {got["score_evals"]} line-search evaluations, gap '
          f'{got["gap"]:.2e}, |score - ref| {abs(got["score"] - ref["score"]):.2e}, max |w - ref| {np.abs(got["w"] - ref["w"]).max():.2e}')
    assert got['converged'] and got['gap'] <= 1e-8
    assert got['iterations'] == ref['iterations'] and got['score_evals'] == ref['score_evals']
    assert abs(got['score'] - ref['score']) <= 1e-9
    assert np.abs(got['w'] - ref['w']).max() <= 1e-6 and abs(got['w'].sum() - 1.0) <= 1e-12


# ---- e. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    from mile_amd import _lib
    eng = _engine()
    lpd = torch.from_numpy(_case(3, 7)).to(DEV)
    w = torch.full((3,), 1.0 / 3, dtype=torch.float64, device=DEV)
    outs = [torch.full(s, 7.0, dtype=torch.float64, device=DEV) for s in ((1,), (7,), (3,), (3, 3))]
    used = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(l=p(lpd), ww=p(w), Cn=3, N=7, o=None, tile=0):
        o = [p(t) for t in outs] + [p(used)] if o is None else o
        return eng.lib.mile_stack_eval(l, ww, Cn, N, *o, tile, None)
    for tag, kw, text in [('null lpd', dict(l=None), 'null'), ('null w', dict(ww=None), 'null'), ('C = 0', dict(Cn=0), 'C out of range'),
                          ('C = 1025', dict(Cn=1025), 'C out of range'), ('N = 0', dict(N=0), 'N out of range'),
                          ('no output', dict(o=[None] * 5), 'no output'), ('tile < 0', dict(tile=-1), 'max_rows_per_tile')]:
        assert call(**kw) == -1, tag
        msg = eng.lib.mile_last_error().decode()
        assert 'mile_stack_eval' in msg and text in msg, (tag, msg)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs) and int(used) == 7      # nothing ran
    with pytest.raises(_lib.MileHipError, match='libmile_hip error -1: mile_stack_eval: C out of range'):
        eng.stack_eval(torch.zeros((1025, 2), dtype=torch.float64), torch.zeros(1025, dtype=torch.float64))
    with pytest.raises(ValueError):
        eng.stack_eval(lpd, w[:2])
    from tests.test_gpu_loo import _fcn_case
    ospec, prob, theta, X, y = _fcn_case('narrow-regr')
    e2 = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    th, Xt, yt = torch.from_numpy(theta[:140]).to(DEV), torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)
    keep = torch.full((2, 70), 7.0, dtype=torch.float64, device=DEV)
    for tag, kw in [('C = 0', dict(Cn=0)), ('C = 1025', dict(Cn=1025)), ('S = 1', dict(S=1)), ('no output', dict(o=None))]:
        Cn, S = kw.get('Cn', 2), kw.get('S', 70)
        o = [None] * 5 if 'o' in kw else [p(keep), None, None, None, None]
        assert e2.lib.mile_chain_loo_stream(e2._h, p(th), Cn, S, p(Xt), p(yt), 70, 1.0, *o, 0, 0, None) == -1, tag
        assert 'mile_chain_loo_stream' in e2.lib.mile_last_error().decode(), tag
    assert e2.lib.mile_chain_loo_stream(e2._h, None, 2, 70, p(Xt), p(yt), 70, 1.0, p(keep), None, None, None, None, 0, 0, None) == -1
    torch.cuda.synchronize()
    assert bool((keep == 7.0).all())
    assert e2.chain_loo_stream_workspace(0, 70, 70) == -1 and e2.chain_loo_stream_workspace(1025, 70, 70) == -1


# ---- f. evaluate.py --stacking ----------------------------------------------------------------------------------------------
def test_evaluate_cli_stacking(tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=120, n_chains=4)      # thinning 10: 12 draws kept per chain
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    _run([ROOT / 'train.py', '-c', tmp_path / 'cfg.yaml', '-d', '1'])
    exp = tmp_path / 'smoke_synthetic'
    _run([ROOT / 'evaluate.py', '-e', exp, '--stacking'])
    m = json.loads((exp / 'metrics.json').read_text())
    z = dict(np.load(exp / 'stacking.npz'))
    (exp / 'stacking.npz').unlink()
    _run([ROOT / 'evaluate.py', '-e', exp])                                            # without the flag: what it always wrote
    plain = json.loads((exp / 'metrics.json').read_text())
    assert not (exp / 'stacking.npz').exists() and not any(k.startswith('stacking') for k in plain)
    assert {k: v for k, v in m.items() if not k.startswith('stacking_')} == plain
    want = ['lppd', 'lppd_equal', 'gain', 'gap', 'iterations', 'converged', 'effective_chains', 'khat_bad', 'weights']
    assert sorted(k for k in m if k.startswith('stacking_')) == sorted('stacking_' + k for k in want)
    assert sorted(z) == ['chain_elpd_loo', 'chain_khat_bad', 'gap', 'n_eval', 'n_train', 'n_train_used', 'weights']
    w = z['weights']
    print(f"cli: weights {np.array2string(w, precision=4)}, lppd {m['lppd']!r}, stacking_lppd_equal {m['stacking_lppd_equal']!r}, "
          f"stacking_lppd {m['stacking_lppd']!r}, gap {m['stacking_gap']:.2e}, {m['stacking_iterations']} Newton steps, khat_bad "
          f"{m['stacking_khat_bad']}")
    assert w.shape == (4,) and abs(w.sum() - 1.0) <= 1e-12 and (w >= 0).all() and m['stacking_weights'] == w.tolist()
    assert abs(m['stacking_lppd_equal'] - m['lppd']) <= 1e-6
    assert m['stacking_converged'] is True and m['stacking_gap'] <= 1e-8 and m['stacking_gap'] == float(z['gap'])
    assert abs(m['stacking_gain'] - (m['stacking_lppd'] - m['stacking_lppd_equal'])) <= 1e-12
    assert abs(m['stacking_effective_chains'] - 1.0 / float((w * w).sum())) <= 1e-12
    eng, samples, x, y = _reload(exp, 'train')
    assert int(z['n_train']) == x.shape[0] and int(z['n_eval']) == m['n_points'] and z['chain_elpd_loo'].shape == (4,)
    rows = eng.chain_loo_stream(torch.from_numpy(samples), torch.from_numpy(x), torch.from_numpy(y), outputs=('elpd_loo', 'khat'))
    s = M.stacking_summary(rows)
    assert np.array_equal(z['chain_elpd_loo'], np.asarray(s['chain_elpd_loo'])) and m['stacking_khat_bad'] == sum(s['chain_khat_bad'])
