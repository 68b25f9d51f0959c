"""The yardsticks of partial dependence on the host (-m "not gpu"): the two forms of tests/pdp_ref.py against each other,
metrics.partial_dependence_dense against the ref, the linear case, pd_grid and partial_dependence_summary on hand-made inputs,
the feature-subset property of the drop rule, and the conditions that the device test puts on its cases (tests/pdp_cases.py)."""
import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import pdp_cases as PC
from tests import pdp_ref as R

torch = pytest.importorskip('torch')

IDS = [c.id for c in PC.CASES]


def _spec(case):
    from mile_amd import ModelSpec
    return ModelSpec(case.F, case.hs, activation=case.act, task=case.task)


@pytest.mark.parametrize('cid', IDS)
def test_update_form_is_substitution(cid):
    """z_0 + (v - x_f) W_0[f] against the column overwritten, both in fp64: the same function to rounding."""
    ref = PC.reference(cid)
    err, top = np.abs(ref['h64'] - ref['sub64']).max(), np.abs(ref['sub64']).max()
    print(f'{cid}: max|update - substitute| = {err:.3e}, max|h| = {top:.3e}')
    assert np.isfinite(ref['h64']).all() and err <= 1e-12 * max(1.0, top)


@pytest.mark.parametrize('cid', IDS)
def test_cases_are_well_chosen(cid):
    """What the device test relies on: the curves are not flat, float32 resolves them, and the update form costs float32 no more
    than substitution does.  No ReLU exclusion is needed: the prediction, unlike the Jacobian, is continuous across the kink."""
    case = PC.BY_ID[cid]
    ref = PC.reference(cid)
    s64, s32 = R.statistics(ref['h64'], case.C), R.statistics(ref['h32'], case.C)
    t64, t32 = R.statistics(ref['sub64'], case.C), R.statistics(ref['sub32'], case.C)
    # the span over the grid: of the draws' curves (0.16 - 8.8 over the eight cases, largest per case) and of their mean pd_mean
    span = (s64['curves'].max(axis=2) - s64['curves'].min(axis=2)).max()
    span_pd = (s64['pd_mean'].max(axis=1) - s64['pd_mean'].min(axis=1)).max()
    print(f'{cid}: largest span over the grid: of a draw\'s curve {span:.3e}, of pd_mean {span_pd:.3e}')
    assert 0.15 <= span <= 9.0, (cid, 'span of the curves', span)
    assert span_pd >= 1e-2, (cid, 'flat pd_mean', span_pd)                   # 1e5 float32 errors of the curves and more
    for k in ('ice_mean', 'ice_sd', 'curves', 'pd_mean', 'pd_sd', 'chain_pd'):
        top, e_upd, e_sub = np.abs(s64[k]).max(), np.abs(s32[k] - s64[k]).max(), np.abs(t32[k] - t64[k]).max()
        print(f'{cid} {k}: float32 restatement, update form {e_upd:.3e} = {e_upd / top:.3e} of the largest, substitute form {e_sub:.3e}, '
              f'ratio {e_upd / e_sub:.2f}')
        assert e_upd <= 1e-6 * top, (cid, k, e_upd, top)
        assert e_upd <= 1.4 * e_sub, (cid, k, e_upd, e_sub)


@pytest.mark.parametrize('cid', IDS)
def test_dense_matches_ref(cid):
    """metrics.partial_dependence_dense of the ModelSpec on the CPU, in batches that split the draws raggedly: fp64 against the
    fp64 substitute form, so the fp32 outputs agree to their rounding and the fp64 ones to 1e-12."""
    from mile_amd import metrics as M
    case = PC.BY_ID[cid]
    _, _, theta, X = PC.problem(cid)
    want = R.statistics(PC.reference(cid)['sub64'], case.C)
    got = M.partial_dependence_dense(_spec(case), torch.from_numpy(theta.copy()).reshape(case.C, case.S, -1), torch.from_numpy(X.copy()),
                                     PC.features_of(cid), torch.from_numpy(PC.grid_of(cid).copy()), batch=2)
    assert set(got) == set(M.PD_OUTPUTS)
    for k in ('ice_mean', 'ice_sd', 'curves'):
        assert got[k].dtype == torch.float32 and got[k].shape == want[k].shape, k
        np.testing.assert_allclose(got[k].numpy(), want[k], rtol=2.0 ** -23, atol=1e-12 * np.abs(want[k]).max(), err_msg=k)
    for k in ('pd_mean', 'pd_sd', 'chain_pd'):
        assert got[k].dtype == torch.float64 and got[k].shape == want[k].shape, k
        np.testing.assert_allclose(got[k].numpy(), want[k], rtol=0, atol=1e-12 * max(1.0, np.abs(want[k]).max()), err_msg=k)
    assert (got['dropped'].numpy() == 0).all() and got['dropped'].dtype == torch.int32 and got['dropped'].shape == (case.N, 3)
    assert (got['chain_draws'].numpy() == case.S).all() and got['chain_draws'].dtype == torch.int64


def test_dense_takes_a_forward_and_refuses_bad_shapes():
    from mile_amd import metrics as M
    case = PC.BY_ID['1-stock']
    _, _, theta, X = PC.problem(case.id)
    spec = _spec(case)
    th, Xt, g = torch.from_numpy(theta.copy()), torch.from_numpy(X.copy()), torch.from_numpy(PC.grid_of(case.id).copy())
    a = M.partial_dependence_dense(spec, th, Xt, (0, 2, 4), g)
    b = M.partial_dependence_dense(lambda t, x: M._fcn_raw(spec, t.to(torch.float64), x.to(torch.float64)), th, Xt, (0, 2, 4), g)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for bad in [dict(features=(0, 0, 4)), dict(features=(0, 2, 5)), dict(features=(0, 2)), dict(features=())]:
        with pytest.raises(ValueError):
            M.partial_dependence_dense(spec, th, Xt, bad['features'], g)


def test_linear_net_has_affine_curves_and_parallel_ice():
    """Case 8, no hidden layer: mu = x W_0[:, 0] + b_0, so each draw's mu curve is affine in v with slope W_0[f, 0], and the ICE
    curves of all rows differ by constants only."""
    case = PC.BY_ID['8-linear']
    ospec, _, theta, X = PC.problem(case.id)
    feats, grid = PC.features_of(case.id), PC.grid_of(case.id).astype(np.float64)
    s = R.statistics(PC.reference(case.id)['h64'], case.C)
    W0 = O.unravel(ospec, theta.astype(np.float64))[0][0]                  # [M, F, 2]
    for i, f in enumerate(feats):
        dv = grid[i] - grid[i][0]
        for p in (0, 1):
            want = W0[:, f, p][:, None] * dv[None, :]
            got = s['curves'][:, i, :, p] - s['curves'][:, i, :1, p]
            assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(s['curves']).max()), (f, p)
    centred = s['ice_mean'] - s['ice_mean'].mean(axis=2, keepdims=True)    # [N, Fs, G, P]
    assert np.abs(centred - centred[:1]).max() <= 1e-13 * max(1.0, np.abs(s['ice_mean']).max())


def test_pd_grid():
    from mile_amd import metrics as M
    x = np.stack([np.arange(101.0), np.arange(101.0)[::-1] ** 2, np.full(101, 3.0)], axis=1).astype(np.float32)
    g = M.pd_grid(x, (0, 1, 2), 5)
    assert g.dtype == torch.float32 and g.shape == (3, 5)
    assert g[0].tolist() == [5.0, 27.5, 50.0, 72.5, 95.0]                      # the quantiles of 0 .. 100 are the levels themselves
    np.testing.assert_allclose(g[1].numpy(), np.quantile(np.arange(101.0) ** 2, np.linspace(0.05, 0.95, 5)), rtol=1e-6)
    assert g[2].tolist() == [3.0] * 5
    lin = M.pd_grid(torch.from_numpy(x), (1,), 3, kind='linspace', lo=0.0, hi=1.0)
    assert lin.tolist() == [[0.0, 5000.0, 10000.0]]
    assert M.pd_grid(x, (0,), 1).tolist() == [[50.0]]
    x[7, 0] = np.inf                                                         # left out: the quantiles of the other 100 values
    np.testing.assert_allclose(M.pd_grid(x, (0,), 2, lo=0.0, hi=1.0).numpy(), [[0.0, 100.0]])
    for bad in [dict(features=(3,), G=5), dict(features=(0,), G=0), dict(features=(0,), G=5, kind='log'), dict(features=(0,), G=5, lo=0.9, hi=0.1)]:
        with pytest.raises(ValueError):
            M.pd_grid(x, **bad)


def test_summary_on_a_hand_made_result():
    """Two features, G = 3, P = 1, two chains, three rows: every number worked out by hand."""
    from mile_amd import metrics as M
    grid = np.array([[0.0, 1.0, 2.0], [10.0, 20.0, 40.0]])
    pd_mean = np.array([[[1.0], [3.0], [5.0]], [[2.0], [2.0], [2.0]]])       # slope 2 on feature 0, flat on feature 1
    pd_sd = np.array([[[0.5], [0.5], [2.0]], [[1.0], [1.0], [1.0]]])
    chain_pd = np.stack([pd_mean + 1.0, pd_mean - 1.0])                      # the chains 2 apart everywhere: sd = sqrt(2)
    ice = np.zeros((3, 2, 3, 1))
    ice[:, 0, :, 0] = [[0.0, 1.0, 2.0], [5.0, 6.0, 7.0], [0.0, 1.0, 2.0]]    # parallel: additive
    ice[:, 1, :, 0] = [[-1.0, 0.0, 1.0], [1.0, 0.0, -1.0], [0.0, 0.0, 0.0]]  # crossing: centred values (-1, 1, 0), 0, (1, -1, 0)
    s = M.partial_dependence_summary({'pd_mean': pd_mean, 'pd_sd': pd_sd, 'chain_pd': chain_pd, 'ice_mean': ice.astype(np.float32)}, grid)
    assert np.allclose(s['importance'], [[2.0], [0.0]]) and np.allclose(s['span'], [[4.0], [0.0]])
    assert np.allclose(s['slope'], [[2.0], [0.0]]) and np.allclose(s['band'], [[1.0], [1.0]])
    assert np.allclose(s['chain_sd'], [[np.sqrt(2.0)], [np.sqrt(2.0)]]) and np.allclose(s['chain_ratio'], [[np.sqrt(2.0)], [np.sqrt(2.0)]])
    assert s['n_chains'] == 2
    assert np.allclose(s['ice_heterogeneity'], [[0.0], [2.0 / 3.0]])          # sd of (-1, 1, 0) is 1, at two of the three grid values
    ice[1] = np.nan                                                          # a row with nothing kept is left out
    one = M.partial_dependence_summary({'pd_mean': pd_mean, 'pd_sd': pd_sd, 'chain_pd': chain_pd[:1], 'ice_mean': ice}, torch.from_numpy(grid))
    assert np.allclose(one['chain_sd'], 0.0) and one['n_chains'] == 1
    assert np.allclose(one['ice_heterogeneity'], [[0.0], [np.sqrt(0.5) * 2.0 / 3.0]])
    # no band (one draw) and no curve at all: no ratio and no NaN, None goes to metrics.json
    import json
    none = M.partial_dependence_summary({'pd_mean': pd_mean, 'pd_sd': np.zeros_like(pd_sd), 'chain_pd': chain_pd}, grid)
    assert none['chain_ratio'] == [[None], [None]] and none['band'] == [[0.0], [0.0]]
    gone = M.partial_dependence_summary({'pd_mean': np.full_like(pd_mean, np.nan), 'pd_sd': np.full_like(pd_sd, np.nan),
                                         'chain_pd': np.full_like(chain_pd, np.nan), 'ice_mean': np.full_like(ice, np.nan)}, grid)
    assert gone['importance'] == [[None], [None]] and gone['ice_heterogeneity'] == [[None], [None]] and gone['n_chains'] == 0
    json.loads(json.dumps(none, allow_nan=False)), json.loads(json.dumps(gone, allow_nan=False))
    with pytest.raises(ValueError):
        M.partial_dependence_summary({'pd_mean': pd_mean, 'pd_sd': pd_sd}, grid[:, :2])


@pytest.mark.parametrize('form', ['update', 'substitute'])
def test_drop_rule_is_per_feature(form):
    """An inf grid value of feature 0 makes every value of feature 0 non-finite and leaves features 2 and 4 alone; a NaN weight
    drops its draw on every feature.  The statistics of a call on [2] are the columns of the call on [0, 2, 4], to the bit, in the
    ref and in metrics.partial_dependence_dense."""
    from mile_amd import metrics as M
    case = PC.BY_ID['1-stock']
    ospec, _, theta, X = PC.problem(case.id)
    theta = theta.copy()
    theta[2, O.param_slices(ospec)[1]['kernel'][0]] = np.nan
    grid = PC.grid_of(case.id).copy()
    grid[0, 3] = np.inf
    full = R.partial_dependence(ospec, theta, X, (0, 2, 4), grid, 1, form=form)
    sub = R.partial_dependence(ospec, theta, X, (2,), grid[1:2], 1, form=form)
    assert (full['dropped'][:, 0] == 7).all() and (full['dropped'][:, 1:] == 1).all()
    assert np.isnan(full['ice_mean'][:, 0]).all() and np.isnan(full['pd_mean'][0]).all() and np.isfinite(full['pd_mean'][1:]).all()
    assert full['chain_draws'].tolist() == [[0, 6, 6]] and np.isnan(full['curves'][2]).all()
    for k in ('ice_mean', 'ice_sd', 'dropped', 'curves', 'chain_pd', 'chain_draws'):
        assert np.array_equal(sub[k][:, 0], full[k][:, 1], equal_nan=True), k
    for k in ('pd_mean', 'pd_sd'):
        assert np.array_equal(sub[k][0], full[k][1]), k
    if form == 'substitute':
        a = M.partial_dependence_dense(_spec(case), torch.from_numpy(theta), torch.from_numpy(X.copy()), (0, 2, 4), torch.from_numpy(grid))
        b = M.partial_dependence_dense(_spec(case), torch.from_numpy(theta), torch.from_numpy(X.copy()), (2,), torch.from_numpy(grid[1:2]))
        assert (a['dropped'].numpy() == full['dropped']).all() and (a['chain_draws'].numpy() == full['chain_draws']).all()
        for k in a:
            i = 0 if k in ('pd_mean', 'pd_sd') else 1
            assert np.array_equal(b[k].select(i, 0).numpy(), a[k].select(i, 1).numpy(), equal_nan=True), k


def test_inf_input_is_dropped_by_the_update_form_only():
    """An inf in column j of a row: substitution takes it out for feature j and keeps the triple; the update form, which is the
    library's definition, has the inf in z_0 already -- inf + (v - inf) w is NaN -- and drops the row for every feature."""
    case = PC.BY_ID['1-stock']
    ospec, _, theta, X = PC.problem(case.id)
    X = X.copy()
    X[5, 2] = np.inf
    grid = PC.grid_of(case.id)
    upd = R.partial_dependence(ospec, theta, X, (0, 2, 4), grid, 1, form='update')
    sub = R.partial_dependence(ospec, theta, X, (0, 2, 4), grid, 1, form='substitute')
    assert upd['dropped'][5].tolist() == [7, 7, 7] and sub['dropped'][5].tolist() == [7, 0, 7]
    assert not np.delete(upd['dropped'], 5, axis=0).any() and not np.delete(sub['dropped'], 5, axis=0).any()
