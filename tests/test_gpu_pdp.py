"""mile_predict_partial_dependence / Engine.predict_partial_dependence against the fp64 NumPy restatement tests/pdp_ref.py on the
cases of tests/pdp_cases.py (-m gpu): every case, every pass and tile size, reproducibility, feature subsets, the null feature,
the linear net, the drop rule, the refusals and the evaluate.py / predict.py CLI.

Bounds, by the method of tests/test_gpu_sens.py.  Per case and output family (ice_mean, ice_sd, curves, pd_mean, pd_sd, chain_pd)
the error of the float32 restatement of the library's arithmetic (pdp_ref.values, form='update', in float32; statistics in fp64)
against fp64 is measured; the device, which does the same arithmetic in another summation order, gets 4x that, plus one unit in
the last place of the output's own format at the family's largest value: 2^-23 for the fp32 outputs (the device rounds its fp64
results to fp32) and 2^-40 for the fp64 ones (a few thousand fp64 additions in another order).  A case whose restatement error
exceeds 1e-3 of a family's largest value has badly chosen inputs and fails as such.  No row is left out for a ReLU kink: the
prediction, unlike its Jacobian, is continuous there."""
import ctypes as C

import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import lenetti_ref as RL
from tests import pdp_cases as PC
from tests import pdp_ref as R
from tests.test_gpu_moments import _agree
from tests.test_gpu_predict import DEV, ROOT, _run
from tests.test_gpu_sens import _engine, _np, _same_bits, _samples

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

FLOAT_KEYS = ('ice_mean', 'ice_sd', 'curves', 'pd_mean', 'pd_sd', 'chain_pd')
ULP = {'ice_mean': 2.0 ** -23, 'ice_sd': 2.0 ** -23, 'curves': 2.0 ** -23, 'pd_mean': 2.0 ** -40, 'pd_sd': 2.0 ** -40, 'chain_pd': 2.0 ** -40}
# (max_draws_per_pass, max_rows_per_tile) of each case's call
CALL = {'1-stock': (3, 32), '2-softmax': (2, 0), '3-k7': (0, 0), '4-b2': (0, 24), '5-deep': (4, 0), '6-wide': (2, 0),
        '7-f70': (0, 16), '8-linear': (3, 10)}


def _call(eng, cid, theta=None, X=None, features=None, grid=None, **kw):
    case = PC.BY_ID[cid]
    _, _, th0, X0 = PC.problem(cid)
    theta = th0 if theta is None else theta
    grid = PC.grid_of(cid) if grid is None else grid
    return eng.predict_partial_dependence(_samples(case, theta), torch.from_numpy(np.ascontiguousarray(X0 if X is None else X)),
                                          PC.features_of(cid) if features is None else features,
                                          torch.from_numpy(np.ascontiguousarray(grid)), **kw)


def _flat(t):
    return t.reshape(-1, t.shape[-1])


@pytest.mark.parametrize('cid', [c.id for c in PC.CASES])
def test_case_against_ref(cid):
    case = PC.BY_ID[cid]
    ref = PC.reference(cid)
    s64, s32 = R.statistics(ref['h64'], case.C), R.statistics(ref['h32'], case.C)
    draws, tile = CALL[cid]
    got = _np(_call(_engine(cid), cid, max_draws_per_pass=draws, max_rows_per_tile=tile))
    P, Fs, G, D = case.hs[-1], 3, PC.G, case.C * case.S
    print(f'{cid}: {case.what}; features {PC.features_of(cid)}, G = {G}')
    assert got['ice_mean'].shape == got['ice_sd'].shape == (case.N, Fs, G, P) and got['dropped'].shape == (case.N, Fs)
    assert got['curves'].shape == (D, Fs, G, P) and got['pd_mean'].shape == got['pd_sd'].shape == (Fs, G, P)
    assert got['chain_pd'].shape == (case.C, Fs, G, P) and got['chain_draws'].shape == (case.C, Fs)
    assert got['ice_mean'].dtype == got['ice_sd'].dtype == got['curves'].dtype == np.float32
    assert got['pd_mean'].dtype == got['pd_sd'].dtype == got['chain_pd'].dtype == np.float64
    assert got['dropped'].dtype == np.int32 and got['chain_draws'].dtype == np.int64
    assert not got['dropped'].any() and (got['chain_draws'] == case.S).all()
    for k in FLOAT_KEYS:
        e32, top = np.abs(s32[k] - s64[k]).max(), np.abs(s64[k]).max()
        err, bound = np.abs(got[k].astype(np.float64) - s64[k]).max(), 4.0 * e32 + ULP[k] * top
        print(f'{cid} {k}: max|out - ref| = {err:.3e}, float32 restatement {e32:.3e}, bound {bound:.3e}, max|ref| = {top:.3e}')
        assert e32 <= 1e-3 * top, (cid, k, 'badly chosen inputs', e32, top)
        assert err <= bound, (cid, k, err, bound)


def test_every_pass_and_tile_size_agrees():
    """Case 1, S = 7 and N = 70: passes of 0 (all) / 3 / 7 draws and tiles of 0 (all) / 32 rows -- a ragged last pass merged by
    Chan's formula, a ragged last tile added to the draws' cells -- against the single-pass, single-tile call."""
    eng = _engine('1-stock')
    one = _call(eng, '1-stock')
    for draws in (0, 3, 7):
        for tile in (0, 32):
            got = _call(eng, '1-stock', max_draws_per_pass=draws, max_rows_per_tile=tile)
            for k in FLOAT_KEYS:
                _agree(f'passes of {draws}, tiles of {tile}: {k}', _flat(got[k]), _flat(one[k]))
            assert torch.equal(got['dropped'], one['dropped']) and torch.equal(got['chain_draws'], one['chain_draws'])


@pytest.mark.parametrize('cid', ['1-stock', '2-softmax'])
def test_same_call_twice_is_bitwise_equal(cid):
    eng = _engine(cid)
    draws, tile = CALL[cid]
    a = _call(eng, cid, max_draws_per_pass=draws, max_rows_per_tile=tile)
    b = _call(eng, cid, max_draws_per_pass=draws, max_rows_per_tile=tile)
    _same_bits(cid, a, b)
    assert all(torch.isfinite(a[k]).all() for k in FLOAT_KEYS)


def test_feature_subset_returns_the_bits_of_the_full_call():
    """Features [2] against the columns of [0, 2, 4], dropped included, with tiles and passes and with the library's choice; and
    with ``want`` naming one output only."""
    eng = _engine('1-stock')
    grid = PC.grid_of('1-stock')
    for kw in (dict(), dict(max_draws_per_pass=3, max_rows_per_tile=32)):
        full = _call(eng, '1-stock', features=(0, 2, 4), **kw)
        sub = _call(eng, '1-stock', features=(2,), grid=grid[1:2], **kw)
        for k in full:
            i = 0 if k in ('pd_mean', 'pd_sd') else 1
            _same_bits(k, {k: sub[k].select(i, 0).contiguous()}, {k: full[k].select(i, 1).contiguous()})
        only = _call(eng, '1-stock', features=(0, 2, 4), want=('pd_sd',), **kw)
        assert list(only) == ['pd_sd']
        _same_bits('want', only, {'pd_sd': full['pd_sd']})


def test_feature_subset_bits_where_the_row_sums_round():
    """Case 2-softmax with the last layer times 8: confident class probabilities from 1e-9 to 1 over 130 rows, so the fp64 row
    sums round and their bits depend on the order of addition.  Features [2] against the columns of [0, 2, 6], and [6, 0] against
    them too: the order must not depend on how many features are selected."""
    cid = '2-softmax'
    ospec, _, theta, _ = PC.problem(cid)
    theta = theta.copy()
    last = O.param_slices(ospec)[-1]
    theta[:, last['bias'][0]:last['bias'][1]] *= 8.0
    theta[:, last['kernel'][0]:last['kernel'][1]] *= 8.0
    grid = PC.grid_of(cid)
    h = R.values(ospec, theta, PC.problem(cid)[3], (0, 2, 6), grid)
    assert np.isfinite(h).all() and h.min() < 1e-6 and h.max() > 0.99     # more than 2^20 between the addends of one sum
    eng = _engine(cid)
    for kw in (dict(), dict(max_draws_per_pass=2, max_rows_per_tile=48)):
        full = _call(eng, cid, theta=theta, features=(0, 2, 6), **kw)
        sub = _call(eng, cid, theta=theta, features=(2,), grid=grid[1:2], **kw)
        two = _call(eng, cid, theta=theta, features=(6, 0), grid=grid[[2, 0]], **kw)
        for k in full:
            i = 0 if k in ('pd_mean', 'pd_sd') else 1
            _same_bits(k, {k: sub[k].select(i, 0).contiguous()}, {k: full[k].select(i, 1).contiguous()})
            _same_bits(k, {k: two[k].select(i, 0).contiguous()}, {k: full[k].select(i, 2).contiguous()})
            _same_bits(k, {k: two[k].select(i, 1).contiguous()}, {k: full[k].select(i, 0).contiguous()})


def test_null_feature_is_constant_over_the_grid():
    """W_0[f, :] = 0 in every draw: z_0 + (v - x) * 0 == z_0, so every output of feature f is the same bits at every grid value,
    and ice_mean there equals that of a call whose grid for f is the rows' own median."""
    cid, f, i = '1-stock', 2, 1
    case = PC.BY_ID[cid]
    ospec, _, theta, X = PC.problem(cid)
    theta = theta.copy()
    k0 = O.param_slices(ospec)[0]['kernel'][0]
    w0 = case.hs[0]
    theta[:, k0 + f * w0:k0 + (f + 1) * w0] = 0.0
    eng = _engine(cid)
    got = _np(_call(eng, cid, theta=theta, max_draws_per_pass=3, max_rows_per_tile=32))
    for k in ('ice_mean', 'ice_sd', 'curves', 'chain_pd'):
        a = got[k][:, i]
        assert (a.view(np.int32 if a.dtype == np.float32 else np.int64) == a[:, :1].view(np.int32 if a.dtype == np.float32 else np.int64)).all(), k
    for k in ('pd_mean', 'pd_sd'):
        assert (got[k][i].view(np.int64) == got[k][i][:1].view(np.int64)).all(), k
    assert np.ptp(got['pd_mean'][0], axis=0).max() > 1e-3                    # the other features still move
    grid = PC.grid_of(cid).copy()
    grid[i, :] = np.float32(np.median(X[:, f]))
    med = _np(_call(eng, cid, theta=theta, grid=grid, max_draws_per_pass=3, max_rows_per_tile=32))
    assert (med['ice_mean'][:, i].view(np.int32) == got['ice_mean'][:, i].view(np.int32)).all()


def test_linear_net_slopes_are_the_weights():
    """Case 8, no hidden layer: each draw's mu and log sigma curves are affine in v with slope W_0[f, p]; the differences of
    ``curves`` along the grid equal the weight times the step to one fp32 ulp of the curve's largest value (the curve is
    rounded to fp32 once, at each end of a difference)."""
    cid = '8-linear'
    ospec, _, theta, _ = PC.problem(cid)
    feats, grid = PC.features_of(cid), PC.grid_of(cid).astype(np.float64)
    got = _np(_call(_engine(cid), cid, max_draws_per_pass=3, max_rows_per_tile=10))
    W0 = O.unravel(ospec, theta.astype(np.float64))[0][0]                  # [M, F, 2]
    top = np.abs(got['curves']).max()
    worst = 0.0
    for i, f in enumerate(feats):
        dv = grid[i] - grid[i][0]
        want = W0[:, f, :][:, None, :] * dv[None, :, None]                   # [M, G, P]
        have = got['curves'][:, i].astype(np.float64) - got['curves'][:, i, :1].astype(np.float64)
        worst = max(worst, np.abs(have - want).max())
    print(f'linear: max|curve differences - weight * step| = {worst:.3e}, one fp32 ulp at the largest = {2.0 ** -23 * top:.3e}')
    assert worst <= 2.0 ** -23 * top


def test_drop_rule():
    """One draw with a NaN weight and one row with an inf input in column 2.  By the library's definition, the update
    z_0 + (v - x_f) W_0[f], the inf is in z_0 already and (v - inf) w does not take it out: the row is dropped for EVERY feature,
    feature 2 included, as pdp_ref's update form has it (its substitute form would keep feature 2).  dropped counts them per
    (row, feature); the other rows and draws are as in a call without them."""
    cid = '1-stock'
    case = PC.BY_ID[cid]
    ospec, _, theta, X = PC.problem(cid)
    theta, X = theta.copy(), X.copy()
    theta[2, O.param_slices(ospec)[1]['kernel'][0]] = np.nan
    X[5, 2] = np.inf
    grid = PC.grid_of(cid)
    want = R.partial_dependence(ospec, theta, X, (0, 2, 4), grid, 1, form='update')
    sub = R.partial_dependence(ospec, theta, X, (0, 2, 4), grid, 1, form='substitute')
    assert want['dropped'][5].tolist() == [7, 7, 7] and sub['dropped'][5].tolist() == [7, 1, 7]
    assert (np.delete(want['dropped'], 5, axis=0) == 1).all()
    eng = _engine(cid)
    got = _call(eng, cid, theta=theta, X=X, max_draws_per_pass=3, max_rows_per_tile=32)
    assert (got['dropped'].cpu().numpy() == want['dropped']).all()
    assert (got['chain_draws'].cpu().numpy() == want['chain_draws']).all() and got['chain_draws'].tolist() == [[6, 6, 6]]
    assert torch.isnan(got['ice_mean'][5]).all() and torch.isnan(got['ice_sd'][5]).all() and torch.isnan(got['curves'][2]).all()
    rows, draws = np.arange(case.N) != 5, np.arange(7) != 2
    clean = eng.predict_partial_dependence(torch.from_numpy(np.delete(theta, 2, axis=0)), torch.from_numpy(np.ascontiguousarray(X[rows])),
                                           (0, 2, 4), torch.from_numpy(grid.copy()))
    assert not clean['dropped'].any() and clean['chain_draws'].tolist() == [[6, 6, 6]]
    sel = torch.from_numpy(rows).to(got['ice_mean'].device)
    for k in ('ice_mean', 'ice_sd'):
        _agree(f'without the draw and the row: {k}', _flat(got[k][sel]), _flat(clean[k]))
    _agree('without the draw and the row: curves', _flat(got['curves'][torch.from_numpy(draws).to(sel.device)]), _flat(clean['curves']))
    for k in ('pd_mean', 'pd_sd', 'chain_pd'):
        _agree(f'without the draw and the row: {k}', _flat(got[k]), _flat(clean[k]))


def test_refusals_leave_the_handle_usable():
    from mile_amd import LeNettiSpec
    from mile_amd.engine import Engine
    cid = '1-stock'
    case = PC.BY_ID[cid]
    _, _, theta, X = PC.problem(cid)
    eng = _engine(cid)
    th, Xt, gr = torch.from_numpy(theta).to(DEV), torch.from_numpy(X).to(DEV), torch.from_numpy(PC.grid_of(cid).copy()).to(DEV)
    mean = torch.empty((case.N, 3, PC.G, 2), dtype=torch.float32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    feats = lambda *f: (C.c_int32 * len(f))(*f)
    ok = dict(th=p(th), C=1, S=7, X=p(Xt), N=case.N, f=feats(0, 2, 4), Fs=3, g=p(gr), G=PC.G, d=0, t=0, out=p(mean))

    def call(e, **kw):
        a = {**ok, **kw}
        return e.lib.mile_predict_partial_dependence(a.get('h', e._h), a['th'], a['C'], a['S'], a['X'], a['N'], a['f'], a['Fs'], a['g'], a['G'], a['d'], a['t'],
                                                     a['out'], None, None, None, None, None, None, None, None)

    big = eng.predict_partial_dependence_workspace(1024, (2 ** 31 - 1) // 1024, case.N, 3, PC.G)
    cases = [('null handle', dict(h=None)), ('null theta', dict(th=None)), ('null X', dict(X=None)), ('null features', dict(f=None)), ('null grid', dict(g=None)),
             ('C = 0', dict(C=0)), ('C = 1025', dict(C=1025)), ('S = 0', dict(S=0)), ('C * S = 2^31', dict(C=2, S=2 ** 30)),
             ('N = 0', dict(N=0)), ('N = 2^30', dict(N=2 ** 30)), ('Fs = 0', dict(Fs=0)), ('Fs = F + 1', dict(Fs=6, f=feats(0, 1, 2, 3, 4, 4))),
             ('feature out of range', dict(f=feats(0, 2, 5))), ('negative feature', dict(f=feats(0, -1, 4))),
             ('repeated feature', dict(f=feats(0, 2, 2))), ('G = 0', dict(G=0)), ('G = 257', dict(G=257)),
             ('negative draws cap', dict(d=-1)), ('negative rows cap', dict(t=-1)), ('no output', dict(out=None)),
             ('output over theta', dict(out=p(th))), ('output over X', dict(out=p(Xt))), ('output over grid', dict(out=p(gr))),
             ('per-draw sums above 1 GiB', dict(C=1024, S=(2 ** 31 - 1) // 1024))]
    for tag, kw in cases:
        rc = call(eng, **kw)
        msg = eng.lib.mile_last_error().decode()
        print(tag, rc, msg)
        assert rc == -1 and 'mile_predict_partial_dependence' in msg, (tag, rc, msg)
        if 'GiB' in tag:
            assert 'fewer features' in msg and big == -1
    W = eng.predict_partial_dependence_workspace
    assert W(0, 7, case.N, 3, 5) == -1 and W(1, 7, case.N, 0, 5) == -1 and W(1, 7, case.N, 6, 5) == -1 and W(1, 7, case.N, 3, 257) == -1
    assert W(1, 7, case.N, 3, 5) > 0 and eng.lib.mile_predict_partial_dependence_workspace(None, 1, 7, case.N, 3, 5) == -1
    with pytest.raises(ValueError):                                       # C * S rows of another width
        eng.predict_partial_dependence(th[:, :-1], Xt, (0, 2, 4), gr)
    with pytest.raises(ValueError):
        eng.predict_partial_dependence(th.reshape(7, 1, 1, -1), Xt, (0, 2, 4), gr)
    with pytest.raises(ValueError):
        eng.predict_partial_dependence(th, Xt[:, :-1], (0, 2, 4), gr)
    with pytest.raises(ValueError):                                       # a grid row per feature
        eng.predict_partial_dependence(th, Xt, (0, 2), gr)
    with pytest.raises(ValueError):
        eng.predict_partial_dependence(th, Xt, (0, 2, 4), gr, want=('mean',))
    a = eng.predict_partial_dependence(th, Xt, (0, 2, 4), gr)
    b = eng.predict_partial_dependence(th, Xt, (0, 2, 4), gr, max_draws_per_pass=1)
    _agree('after the refusals', _flat(b['ice_mean']), _flat(a['ice_mean']))
    assert torch.isfinite(a['ice_mean']).all() and torch.isfinite(a['pd_sd']).all()
    # a net too wide for LDS: one row's z_0 (14 081 floats) and one pseudo-row's two buffers (2 x 14 084) take 165 KiB of the 160
    from mile_amd import ModelSpec
    wspec = ModelSpec(case.F, (14080, 2))
    wide = Engine(wspec, Xt[:8], torch.zeros(8, device=DEV), device=DEV)
    tw = torch.zeros((1, wspec.n_params), dtype=torch.float32, device=DEV)
    rc = call(wide, th=p(tw), S=1)
    msg = wide.lib.mile_last_error().decode()
    print('too wide', rc, msg)
    assert rc == -1 and 'mile_predict_partial_dependence' in msg and 'LDS' in msg
    assert wide.predict_partial_dependence_workspace(1, 1, case.N, 3, PC.G) == -1
    assert torch.isfinite(wide.predict(tw, Xt)).all()                     # the handle goes on
    del wide, tw
    # a LeNetti handle: pixels have no partial dependence here; its other evaluation calls go on
    ospec = RL.LeNettiSpec(3, 9, 11, 2, activation='tanh', task='regr')
    prob = RL.synthetic_problem(ospec, 20, 3, seed=6)
    img = Engine(LeNettiSpec(3, 9, 11, 2, activation='tanh', task='regr'), torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV)
    t3, X3 = torch.from_numpy(prob['theta0']).to(DEV), torch.from_numpy(prob['X']).reshape(20, -1).contiguous().to(DEV)
    out = torch.empty((20, 3, PC.G, 2), dtype=torch.float32, device=DEV)
    rc = call(img, th=p(t3), S=3, X=p(X3), N=20, out=p(out))
    msg = img.lib.mile_last_error().decode()
    print('lenetti', rc, msg)
    assert rc == -1 and 'mile_predict_partial_dependence' in msg and 'FCN' in msg
    assert img.predict_partial_dependence_workspace(1, 3, 20, 3, PC.G) == -1
    assert torch.isfinite(img.predict_moments(t3, torch.from_numpy(prob['X']))).all()


def test_cli(tmp_path):
    """train.py on the smoke experiment, evaluate.py --partial-dependence 5 (keys, shapes, equal to the Engine on the same split
    and grid), then predict.py --partial-dependence 5 with and without --normalized: the two differ by the factors of the
    normalisation."""
    import json
    import yaml
    from mile_amd import metrics as M
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=30, n_chains=4)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    _run([ROOT / 'train.py', '-c', tmp_path / 'cfg.yaml', '-d', '1'])
    exp = tmp_path / 'smoke_synthetic'
    _run([ROOT / 'evaluate.py', '-e', exp, '--split', 'test', '--partial-dependence', '5'])
    from mile_amd.callbacks import load_samples_from_dir
    from mile_amd.config import Config
    from mile_amd.trainer import BDETrainer
    conf = Config.from_file(exp / 'config.yaml').replace(logging=False)
    tr = BDETrainer.__new__(BDETrainer)
    tr.build_model(conf)
    spec = tr.prob_model.spec
    samples = load_samples_from_dir(exp / conf.training.sampler._dir_name, spec)
    x = np.ascontiguousarray(tr.loader.test_x).reshape(len(tr.loader.test_x), -1)
    N, F, P, Cn, D, G = len(x), spec.in_features, spec.hidden_structure[-1], samples.shape[0], samples.shape[0] * samples.shape[1], 5
    metrics = json.loads((exp / 'metrics.json').read_text())
    for k in ('pd_importance', 'pd_span', 'pd_slope', 'pd_band', 'pd_chain_sd', 'pd_chain_ratio', 'pd_ice_heterogeneity'):
        assert np.asarray(metrics[k]).shape == (F, P), k
    assert metrics['pd_dropped'] == 0 and metrics['pd_features'] == list(range(F)) and metrics['pd_grid_points'] == G
    arr = np.load(exp / 'partial_dependence.npz')
    assert arr['grid'].shape == (F, G) and arr['grid'].dtype == np.float32
    assert arr['ice_mean'].shape == arr['ice_sd'].shape == (N, F, G, P) and arr['dropped'].shape == (N, F)
    assert arr['curves'].shape == (D, F, G, P) and arr['pd_mean'].shape == arr['pd_sd'].shape == (F, G, P)
    assert arr['chain_pd'].shape == (Cn, F, G, P) and arr['chain_draws'].shape == (Cn, F)
    assert (arr['feature_index'] == np.arange(F)).all() and (('feature_names' not in arr.files) or arr['feature_names'].shape == (F,))
    eng = tr.prob_model.engine(torch.from_numpy(np.ascontiguousarray(tr.loader.train_x).reshape(len(tr.loader.train_x), -1)),
                               torch.from_numpy(np.ascontiguousarray(tr.loader.train_y)), device=DEV)
    grid = M.pd_grid(x, range(F), G)
    assert (arr['grid'] == grid.numpy()).all()
    same = _np(eng.predict_partial_dependence(torch.from_numpy(samples), torch.from_numpy(x), range(F), grid))
    for k in same:
        assert np.array_equal(arr[k], same[k], equal_nan=True), k            # the same call on the same inputs: the same bits
    np.testing.assert_allclose(metrics['pd_importance'], same['pd_mean'].std(axis=1, ddof=1), rtol=1e-12)
    # a selection of features
    _run([ROOT / 'evaluate.py', '-e', exp, '--split', 'test', '--partial-dependence', '--pd-features', '1'])
    sel = np.load(exp / 'partial_dependence.npz')
    assert sel['grid'].shape == (1, 20) and sel['feature_index'].tolist() == [1] and sel['pd_mean'].shape == (1, 20, P)
    # predict.py: the network's units with --normalized, the table's without
    norm = np.load(exp / 'normalization.npz')
    raw = (x * norm['x_std'] + norm['x_mean']).astype(np.float32)
    seen = np.ascontiguousarray(((raw - norm['x_mean']) / norm['x_std']).astype(np.float32))
    np.save(tmp_path / 'raw_x.npy', raw)
    np.save(tmp_path / 'seen_x.npy', seen)
    _run([ROOT / 'predict.py', '-e', exp, '-i', tmp_path / 'seen_x.npy', '-o', tmp_path / 'net.npz', '--normalized', '--partial-dependence', '5'])
    net = np.load(tmp_path / 'net.npz')
    g_net = M.pd_grid(seen, range(F), G)
    direct = _np(eng.predict_partial_dependence(torch.from_numpy(samples), torch.from_numpy(seen), range(F), g_net))
    assert (net['pd_grid'] == g_net.numpy()).all()
    for k in ('ice_mean', 'ice_sd'):
        assert (net[f'pd_{k}'] == direct[k]).all(), k
    assert (net['pd_mean'] == direct['pd_mean']).all() and (net['pd_sd'] == direct['pd_sd']).all()
    _run([ROOT / 'predict.py', '-e', exp, '-i', tmp_path / 'raw_x.npy', '-o', tmp_path / 'raw.npz', '--partial-dependence', '5'])
    back = np.load(tmp_path / 'raw.npz')
    y_std, y_mean = float(norm['y_std'].reshape(-1)[0]), float(norm['y_mean'].reshape(-1)[0])
    x_std, x_mean = norm['x_std'].astype(np.float64).reshape(F), norm['x_mean'].astype(np.float64).reshape(F)
    np.testing.assert_allclose(back['pd_grid'], net['pd_grid'].astype(np.float64) * x_std[:, None] + x_mean[:, None], rtol=1e-5, atol=0)
    scale, shift = np.array([y_std, 1.0]), np.array([y_mean, np.log(y_std)])  # mu back in target units, log sigma shifted by log y_std
    for k in ('pd_ice_mean', 'pd_mean'):
        want = net[k].astype(np.float64) * scale + shift
        np.testing.assert_allclose(back[k], want, rtol=1e-5, atol=0, err_msg=k)
    for k in ('pd_ice_sd', 'pd_sd'):
        want = net[k].astype(np.float64) * scale
        np.testing.assert_allclose(back[k], want, rtol=1e-5, atol=0, err_msg=k)
    assert sorted(f for f in back.files if not f.startswith('pd_')) == ['aleatoric_var', 'dropped', 'epistemic_var', 'mean']
