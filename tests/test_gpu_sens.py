"""mile_predict_sensitivities / Engine.predict_sensitivities against the fp64 NumPy restatement tests/sens_ref.py on the cases
of tests/sens_cases.py (-m gpu): every case, every pass and tile size, reproducibility, the linear and the dead net, the drop
rule, the refusals and the evaluate.py / predict.py CLI.

Bounds, by the method of tests/test_gpu_moments.py.  Per case and output family (mean, sd, chain_ape, chain_abs) the error of
the float32 restatement of the Jacobian chain (sens_ref.jacobians in float32, statistics in fp64) against fp64 is measured;
the device, which does the same arithmetic in another summation order, gets 4x that, plus one unit in the last place of the
output's own format at the family's largest value: 2^-23 for the fp32 outputs (the device rounds its fp64 mean and sd to fp32;
where the Jacobian is exact, as in the linear case, nothing else is left) and 2^-40 for the fp64 chain outputs (a few thousand
fp64 additions in another order).  A case whose restatement error exceeds 1e-3 of a family's largest value, or whose reference
max|J| is below 1e-3, has badly chosen inputs and fails as such.

pos * k must equal the reference's count of positive draws, except in columns where some kept draw has |J| below 16
restatement errors of J: there it may differ by at most the number of such draws.

ReLU cases: a hidden pre-activation within rounding of 0 takes another mask in fp32 than in fp64 and the row's Jacobian differs
discretely, so rows where some draw has |z| < 4e-6 (sum_i |a_i W_ij| + |b_j|) are left out of the per-row comparison (at most 5 %
of a case's rows, asserted), and the chain outputs are compared over the remaining rows through a second device call on them."""
import ctypes as C

import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import lenetti_ref as RL
from tests import sens_cases as SC
from tests import sens_ref as R
from tests.test_gpu_moments import _agree
from tests.test_gpu_predict import DEV, ROOT, _run

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

FLOAT_KEYS = ('mean', 'sd', 'pos', 'chain_ape', 'chain_abs')
ULP = {'mean': 2.0 ** -23, 'sd': 2.0 ** -23, 'chain_ape': 2.0 ** -40, 'chain_abs': 2.0 ** -40}
# (max_draws_per_pass, max_rows_per_tile) of each case's call
CALL = {'1-stock': (3, 32), '2-softmax': (2, 0), '3-k7': (0, 0), '4-b2': (0, 24), '5-deep': (4, 0), '6-wide': (2, 0),
        '7-f70': (0, 16), '8-linear': (3, 10)}


def _engine(cid):
    from mile_amd import ModelSpec
    from mile_amd.engine import Engine
    case = SC.BY_ID[cid]
    _, prob, _, _ = SC.problem(cid)
    spec = ModelSpec(case.F, case.hs, activation=case.act, task=case.task)
    return Engine(spec, torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV)


def _samples(case, theta):
    return torch.from_numpy(np.ascontiguousarray(theta)).reshape(case.C, -1, theta.shape[-1])


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same_bits(tag, a, b):
    for k in a:
        assert torch.equal(a[k].view(torch.int32 if a[k].dtype == torch.float32 else torch.int64) if a[k].is_floating_point() else a[k],
                           b[k].view(torch.int32 if b[k].dtype == torch.float32 else torch.int64) if b[k].is_floating_point() else b[k]), (tag, k)


@pytest.mark.parametrize('cid', [c.id for c in SC.CASES])
def test_case_against_ref(cid):
    case = SC.BY_ID[cid]
    _, _, theta, X = SC.problem(cid)
    ref = SC.reference(cid)
    keep = ~ref['near']
    print(f'{cid}: {case.what}; {int((~keep).sum())} of {case.N} rows left out for a pre-activation within rounding of 0')
    assert (~keep).sum() <= 0.05 * case.N
    s64 = R.statistics(ref['raw64'][:, keep], ref['J64'][:, keep], case.C)
    s32 = R.statistics(ref['raw32'][:, keep], ref['J32'][:, keep], case.C)
    top_J, e_J = np.abs(ref['J64']).max(), np.abs(ref['J32'][:, keep] - ref['J64'][:, keep]).max()
    print(f'{cid}: max|J| = {top_J:.3e}, float32 restatement of J {e_J:.3e}')
    assert top_J >= 1e-3, (cid, 'badly chosen inputs', top_J)
    eng = _engine(cid)
    draws, tile = CALL[cid]
    got = _np(eng.predict_sensitivities(_samples(case, theta), torch.from_numpy(X), max_draws_per_pass=draws, max_rows_per_tile=tile))
    P = case.hs[-1]
    assert got['mean'].shape == got['sd'].shape == got['pos'].shape == (case.N, P, case.F) and got['dropped'].shape == (case.N,)
    assert got['chain_ape'].shape == got['chain_abs'].shape == (case.C, P, case.F) and got['chain_kept'].shape == (case.C,)
    assert got['mean'].dtype == np.float32 and got['chain_ape'].dtype == np.float64
    assert got['dropped'].dtype == np.int32 and got['chain_kept'].dtype == np.int64
    assert not got['dropped'].any() and (got['chain_kept'] == case.S * case.N).all()
    chain = got
    if not keep.all():                                                   # the chain outputs over the rows that are compared
        chain = _np(eng.predict_sensitivities(_samples(case, theta), torch.from_numpy(np.ascontiguousarray(X[keep])),
                                              max_draws_per_pass=draws, max_rows_per_tile=tile))
        assert (chain['chain_kept'] == case.S * keep.sum()).all()
    for k in ('mean', 'sd', 'chain_ape', 'chain_abs'):
        e32, top = np.abs(s32[k] - s64[k]).max(), np.abs(s64[k]).max()
        have = got[k][keep] if k in ('mean', 'sd') else chain[k]
        err, bound = np.abs(have.astype(np.float64) - s64[k]).max(), 4.0 * e32 + ULP[k] * top
        print(f'{cid} {k}: max|out - ref| = {err:.3e}, float32 restatement {e32:.3e}, bound {bound:.3e}, max|ref| = {top:.3e}')
        assert e32 <= 1e-3 * top, (cid, k, 'badly chosen inputs', e32, top)
        assert err <= bound, (cid, k, err, bound)
    k_dev = (case.C * case.S - got['dropped'][keep]).astype(np.float64)[:, None, None]
    cnt = got['pos'][keep].astype(np.float64) * k_dev
    assert np.abs(cnt - np.rint(cnt)).max() < 1e-3
    small = (np.abs(ref['J64'][:, keep]) < 16.0 * e_J).sum(axis=0)      # kept draws of a column whose sign rounding may turn
    diff = np.abs(np.rint(cnt).astype(np.int64) - s64['count_pos'])
    print(f'{cid} pos: {int((diff > 0).sum())} columns differ in their count, {int((small > 0).sum())} hold a draw below {16.0 * e_J:.3e}')
    assert (diff <= small).all(), (cid, 'pos', int(diff.max()))


def test_every_pass_and_tile_size_agrees():
    """Case 1, S = 7 and N = 70: passes of 0 (all) / 3 / 7 draws and tiles of 0 (all) / 32 rows -- a ragged last pass merged by
    Chan's formula, a ragged last tile -- against the single-pass, single-tile call."""
    case = SC.BY_ID['1-stock']
    _, _, theta, X = SC.problem(case.id)
    eng = _engine(case.id)
    th, Xt = _samples(case, theta), torch.from_numpy(X)
    one = eng.predict_sensitivities(th, Xt)
    for draws in (0, 3, 7):
        for tile in (0, 32):
            got = eng.predict_sensitivities(th, Xt, max_draws_per_pass=draws, max_rows_per_tile=tile)
            for k in FLOAT_KEYS:
                _agree(f'passes of {draws}, tiles of {tile}: {k}', got[k].reshape(-1, case.F), one[k].reshape(-1, case.F))
            assert torch.equal(got['dropped'], one['dropped']) and torch.equal(got['chain_kept'], one['chain_kept'])


@pytest.mark.parametrize('cid', ['1-stock', '2-softmax'])
def test_same_call_twice_is_bitwise_equal(cid):
    case = SC.BY_ID[cid]
    _, _, theta, X = SC.problem(cid)
    eng = _engine(cid)
    draws, tile = CALL[cid]
    a = eng.predict_sensitivities(_samples(case, theta), torch.from_numpy(X), max_draws_per_pass=draws, max_rows_per_tile=tile)
    b = eng.predict_sensitivities(_samples(case, theta), torch.from_numpy(X), max_draws_per_pass=draws, max_rows_per_tile=tile)
    _same_bits(cid, a, b)
    assert torch.isfinite(a['mean']).all() and torch.isfinite(a['chain_ape']).all()


def test_linear_net_returns_its_weights():
    """Case 8, no hidden layer: each draw's J is W_0 transposed, bit for bit on every row -- through S = 1 calls, where sd == 0
    and pos is 0 or 1 -- and the mean over all draws is the mean of the weights."""
    case = SC.BY_ID['8-linear']
    ospec, _, theta, X = SC.problem(case.id)
    eng = _engine(case.id)
    Xt = torch.from_numpy(X)
    W0 = np.swapaxes(O.unravel(ospec, theta)[0][0], 1, 2)               # [M, P, F]
    for s in range(theta.shape[0]):
        got = _np(eng.predict_sensitivities(torch.from_numpy(theta[s:s + 1].copy()), Xt))
        assert (got['mean'].view(np.int32) == np.broadcast_to(W0[s], got['mean'].shape).view(np.int32)).all(), s
        assert (got['sd'] == 0).all() and (got['pos'] == (W0[s] > 0).astype(np.float32)).all()
        assert (got['chain_ape'][0] == W0[s].astype(np.float64)).all() and (got['chain_abs'][0] == np.abs(W0[s]).astype(np.float64)).all()
    got = _np(eng.predict_sensitivities(_samples(case, theta), Xt, max_draws_per_pass=3, max_rows_per_tile=10))
    want = W0.astype(np.float64).mean(axis=0)
    err = np.abs(got['mean'].astype(np.float64) - want).max()
    print(f'linear: max|mean - mean of the weights| = {err:.3e}, one fp32 ulp at the largest = {2.0 ** -23 * np.abs(want).max():.3e}')
    assert err <= 2.0 ** -23 * np.abs(want).max()
    np.testing.assert_allclose(got['chain_ape'], W0.astype(np.float64).reshape(case.C, case.S, *W0.shape[1:]).mean(axis=1), rtol=1e-14, atol=0)


def test_dead_net_has_no_sensitivity():
    """Case 1 with every hidden bias at -10 and inputs in [0, 1]: no unit is ever active, every mask is 0 and every output
    exactly 0."""
    case = SC.BY_ID['1-stock']
    ospec, _, theta, X = SC.problem(case.id)
    theta, X = theta.copy(), np.minimum(np.abs(X), 1.0).astype(np.float32)
    for ent in O.param_slices(ospec)[:-1]:
        theta[:, ent['bias'][0]:ent['bias'][1]] = -10.0
    _, zs, _ = O.mlp_forward(ospec, theta.astype(np.float64), X.astype(np.float64), keep=True)
    assert all((z < -1.0).all() for z in zs[:-1])                       # dead with room to spare in any precision
    got = _np(_engine(case.id).predict_sensitivities(_samples(case, theta), torch.from_numpy(X), max_draws_per_pass=3))
    for k in FLOAT_KEYS:
        assert (got[k] == 0).all(), k
    assert not got['dropped'].any() and int(got['chain_kept'][0]) == case.S * case.N


def test_drop_rule():
    """One draw with a NaN weight and one row with an inf input: dropped counts them per row, the other rows and draws are as in a
    call without them, chain_kept matches."""
    case = SC.BY_ID['1-stock']
    ospec, _, theta, X = SC.problem(case.id)
    theta, X = theta.copy(), X.copy()
    theta[2, O.param_slices(ospec)[1]['kernel'][0]] = np.nan
    X[5, 3] = np.inf
    want = R.sensitivities(ospec, theta, X, 1)
    assert want['dropped'][5] == 7 and (np.delete(want['dropped'], 5) == 1).all()
    eng = _engine(case.id)
    got = eng.predict_sensitivities(torch.from_numpy(theta), torch.from_numpy(X), max_draws_per_pass=3, max_rows_per_tile=32)
    assert (got['dropped'].cpu().numpy() == want['dropped']).all()
    assert int(got['chain_kept'][0]) == int(want['chain_kept'][0]) == 6 * 69
    for k in ('mean', 'sd', 'pos'):
        assert torch.isnan(got[k][5]).all(), k
    rows = np.arange(case.N) != 5
    clean = eng.predict_sensitivities(torch.from_numpy(np.delete(theta, 2, axis=0)), torch.from_numpy(np.ascontiguousarray(X[rows])))
    assert not clean['dropped'].any() and int(clean['chain_kept'][0]) == 6 * 69
    sel = torch.from_numpy(rows).to(got['mean'].device)
    for k in ('mean', 'sd', 'pos'):
        _agree(f'without the draw and the row: {k}', got[k][sel].reshape(-1, case.F), clean[k].reshape(-1, case.F))
    for k in ('chain_ape', 'chain_abs'):
        _agree(f'without the draw and the row: {k}', got[k].reshape(-1, case.F), clean[k].reshape(-1, case.F))


def test_refusals_leave_the_handle_usable():
    from mile_amd import LeNettiSpec
    from mile_amd.engine import Engine
    case = SC.BY_ID['1-stock']
    _, _, theta, X = SC.problem(case.id)
    eng = _engine(case.id)
    th, Xt = torch.from_numpy(theta).to(DEV), torch.from_numpy(X).to(DEV)
    mean = torch.empty((case.N, 2, case.F), dtype=torch.float32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(e, th_, C_, S_, X_, N_, mean_):
        return e.lib.mile_predict_sensitivities(e._h, th_, C_, S_, X_, N_, 0, 0, mean_, None, None, None, None, None, None, None)

    for tag, args in [('null theta', (None, 1, 7, p(Xt), case.N, p(mean))), ('null X', (p(th), 1, 7, None, case.N, p(mean))),
                      ('C = 0', (p(th), 0, 7, p(Xt), case.N, p(mean))), ('S = 0', (p(th), 1, 0, p(Xt), case.N, p(mean))),
                      ('N = 0', (p(th), 1, 7, p(Xt), 0, p(mean))), ('no output', (p(th), 1, 7, p(Xt), case.N, None)),
                      ('output over theta', (p(th), 1, 7, p(Xt), case.N, p(th))), ('output over X', (p(th), 1, 7, p(Xt), case.N, p(Xt)))]:
        rc = call(eng, *args)
        msg = eng.lib.mile_last_error().decode()
        print(tag, rc, msg)
        assert rc == -1 and 'mile_predict_sensitivities' in msg, (tag, rc, msg)
    assert eng.predict_sensitivities_workspace(0, 7, case.N) == -1 and eng.predict_sensitivities_workspace(1, 7, case.N) > 0
    with pytest.raises(ValueError):                                       # C * S rows of another width
        eng.predict_sensitivities(th[:, :-1], Xt)
    with pytest.raises(ValueError):
        eng.predict_sensitivities(th.reshape(7, 1, 1, -1), Xt)
    a = eng.predict_sensitivities(th, Xt)
    b = eng.predict_sensitivities(th, Xt, max_draws_per_pass=1)
    _agree('after the refusals', b['mean'].reshape(-1, case.F), a['mean'].reshape(-1, case.F))
    assert torch.isfinite(a['mean']).all()
    # a LeNetti handle: pixels have no sensitivities here; its other evaluation calls go on
    ospec = RL.LeNettiSpec(3, 9, 11, 2, activation='tanh', task='regr')
    prob = RL.synthetic_problem(ospec, 20, 3, seed=6)
    img = Engine(LeNettiSpec(3, 9, 11, 2, activation='tanh', task='regr'), torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV)
    t3, X3 = torch.from_numpy(prob['theta0']).to(DEV), torch.from_numpy(prob['X']).reshape(20, -1).contiguous().to(DEV)
    out = torch.empty((20, 2, X3.shape[1]), dtype=torch.float32, device=DEV)
    rc = call(img, p(t3), 1, 3, p(X3), 20, p(out))
    msg = img.lib.mile_last_error().decode()
    print('lenetti', rc, msg)
    assert rc == -1 and 'mile_predict_sensitivities' in msg and 'FCN' in msg
    assert img.predict_sensitivities_workspace(1, 3, 20) == -1
    assert torch.isfinite(img.predict_moments(t3, torch.from_numpy(prob['X']))).all()


def test_cli(tmp_path):
    """train.py on the smoke experiment, evaluate.py --sensitivities (keys, shapes, equal to the Engine on the same split), then
    predict.py --sensitivities with and without --normalized: the two differ by the factors of the normalisation."""
    import json
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=30, n_chains=4)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    _run([ROOT / 'train.py', '-c', tmp_path / 'cfg.yaml', '-d', '1'])
    exp = tmp_path / 'smoke_synthetic'
    _run([ROOT / 'evaluate.py', '-e', exp, '--split', 'test', '--sensitivities'])
    from mile_amd.callbacks import load_samples_from_dir
    from mile_amd.config import Config
    from mile_amd.trainer import BDETrainer
    conf = Config.from_file(exp / 'config.yaml').replace(logging=False)
    tr = BDETrainer.__new__(BDETrainer)
    tr.build_model(conf)
    spec = tr.prob_model.spec
    samples = load_samples_from_dir(exp / conf.training.sampler._dir_name, spec)
    x = np.ascontiguousarray(tr.loader.test_x).reshape(len(tr.loader.test_x), -1)
    N, F, P, Cn = len(x), spec.in_features, spec.hidden_structure[-1], samples.shape[0]
    metrics = json.loads((exp / 'metrics.json').read_text())
    for k in ('sens_ape', 'sens_importance', 'sens_chain_sd', 'sens_decided', 'sens_ranking'):
        assert np.asarray(metrics[k]).shape == (P, F), k
    assert metrics['sens_dropped'] == 0 and all(sorted(r) == list(range(F)) for r in metrics['sens_ranking'])
    arr = np.load(exp / 'sensitivities.npz')
    assert arr['mean'].shape == arr['sd'].shape == arr['pos'].shape == (N, P, F) and arr['dropped'].shape == (N,)
    assert arr['chain_ape'].shape == arr['chain_abs'].shape == (Cn, P, F) and arr['chain_kept'].shape == (Cn,)
    assert ('feature_index' in arr.files and (arr['feature_index'] == np.arange(F)).all()) or arr['feature_names'].shape == (F,)
    eng = tr.prob_model.engine(torch.from_numpy(np.ascontiguousarray(tr.loader.train_x).reshape(len(tr.loader.train_x), -1)),
                               torch.from_numpy(np.ascontiguousarray(tr.loader.train_y)), device=DEV)
    same = _np(eng.predict_sensitivities(torch.from_numpy(samples), torch.from_numpy(x)))
    for k in same:
        assert (arr[k] == same[k]).all(), k                              # the same call on the same inputs: the same bits
    np.testing.assert_allclose(metrics['sens_importance'], same['chain_abs'].mean(axis=0), rtol=1e-12)
    # predict.py: the network's units with --normalized, the table's without
    norm = np.load(exp / 'normalization.npz')
    # a table in the units of the raw data, and the rows the network sees for it: predict.py's own normalisation, so that both
    # runs forward the same bits (rows that went through x * std + mean and back would be moved by an ulp, and a ReLU mask could turn)
    raw = (x * norm['x_std'] + norm['x_mean']).astype(np.float32)
    seen = np.ascontiguousarray(((raw - norm['x_mean']) / norm['x_std']).astype(np.float32))
    np.save(tmp_path / 'raw_x.npy', raw)
    np.save(tmp_path / 'seen_x.npy', seen)
    _run([ROOT / 'predict.py', '-e', exp, '-i', tmp_path / 'seen_x.npy', '-o', tmp_path / 'net.npz', '--normalized', '--sensitivities'])
    net = np.load(tmp_path / 'net.npz')
    direct = _np(eng.predict_sensitivities(torch.from_numpy(samples), torch.from_numpy(seen)))
    for k in ('mean', 'sd', 'pos', 'dropped'):
        assert (net[f'sens_{k}'] == direct[k]).all(), k
    _run([ROOT / 'predict.py', '-e', exp, '-i', tmp_path / 'raw_x.npy', '-o', tmp_path / 'raw.npz', '--sensitivities'])
    back = np.load(tmp_path / 'raw.npz')
    factor = np.ones((P, F)) / norm['x_std'].astype(np.float64).reshape(1, F)     # d mu / d x_f: y_std / x_std_f; d log sigma / d x_f: 1 / x_std_f
    factor[0] *= float(norm['y_std'].reshape(-1)[0])
    for k in ('mean', 'sd'):
        np.testing.assert_allclose(back[f'sens_{k}'], net[f'sens_{k}'].astype(np.float64) * factor, rtol=1e-5, atol=0, err_msg=k)
    assert (back['sens_pos'] == net['sens_pos']).all() and (back['sens_dropped'] == net['sens_dropped']).all()
    assert sorted(f for f in back.files if not f.startswith('sens_')) == ['aleatoric_var', 'dropped', 'epistemic_var', 'mean']
