"""The yardsticks of the input sensitivities on the host (-m "not gpu"): tests/sens_ref.py against torch autograd and central
differences, metrics.sensitivities_dense against sens_ref, sensitivity_summary on a hand-made result, the linear case, and the
conditions that the device test puts on its cases (tests/sens_cases.py)."""
import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import sens_cases as SC
from tests import sens_ref as R

torch = pytest.importorskip('torch')


def _spec(case):
    from mile_amd import ModelSpec
    return ModelSpec(case.F, case.hs, activation=case.act, task=case.task)


@pytest.mark.parametrize('cid', ['1-stock', '2-softmax', '3-k7', '7-f70'])
def test_ref_matches_autograd(cid):
    """relu / tanh / sigmoid, (mu, log sigma) and softmax heads: every (draw, row) of a few against
    torch.autograd.functional.jacobian of the fp64 forward (away from ReLU's kink the two are the same derivative)."""
    from mile_amd import metrics as M
    case = SC.BY_ID[cid]
    ospec, _, theta, X = SC.problem(cid)
    spec = _spec(case)
    J = SC.reference(cid)['J64']
    th, Xt = torch.from_numpy(theta.astype(np.float64)), torch.from_numpy(X.astype(np.float64))

    def head(x, s):
        out = M.predict(spec, th[s:s + 1], x[None])[0, 0]
        return out if case.task == 'regr' else torch.softmax(out, dim=-1)

    worst = 0.0
    for s in (0, theta.shape[0] - 1):
        for n in (0, 1, case.N - 1):
            ref = torch.autograd.functional.jacobian(lambda x: head(x, s), Xt[n]).numpy()
            worst = max(worst, np.abs(J[s, n] - ref).max())
    print(f'{cid}: max|J - autograd| = {worst:.3e}, max|J| = {np.abs(J).max():.3e}')
    assert worst <= 1e-12 * max(1.0, np.abs(J).max())


@pytest.mark.parametrize('cid', ['2-softmax', '3-k7', '7-f70'])
def test_ref_matches_central_differences(cid):
    """The smooth activations: central differences with h = 1e-5 in fp64 have truncation error h^2 f''' / 6 and rounding error
    eps / h, both about 1e-10 of the outputs' scale; 1e-7 leaves room for the third derivatives of these nets."""
    ospec, _, theta, X = SC.problem(cid)
    J = SC.reference(cid)['J64']
    fd = R.finite_difference(ospec, theta, X[:9])
    err = np.abs(J[:, :9] - fd).max()
    print(f'{cid}: max|J - central differences| = {err:.3e}, max|J| = {np.abs(J).max():.3e}')
    assert err < 1e-7 * max(1.0, np.abs(J).max())


@pytest.mark.parametrize('cid', [c.id for c in SC.CASES])
def test_dense_matches_ref(cid):
    """metrics.sensitivities_dense on the CPU, in batches that split a chain raggedly: fp64 against fp64, so the fp32 outputs
    agree to their rounding and the fp64 ones to 1e-12."""
    from mile_amd import metrics as M
    case = SC.BY_ID[cid]
    _, _, theta, X = SC.problem(cid)
    ref = SC.reference(cid)
    want = R.statistics(ref['raw64'], ref['J64'], case.C)
    got = M.sensitivities_dense(_spec(case), torch.from_numpy(theta.copy()).reshape(case.C, case.S, -1), torch.from_numpy(X.copy()), batch=2)
    P = case.hs[-1]
    assert got['mean'].shape == got['sd'].shape == got['pos'].shape == (case.N, P, case.F)
    assert got['chain_ape'].shape == got['chain_abs'].shape == (case.C, P, case.F) and got['chain_kept'].shape == (case.C,)
    assert got['mean'].dtype == torch.float32 and got['chain_ape'].dtype == torch.float64
    assert got['dropped'].dtype == torch.int32 and got['chain_kept'].dtype == torch.int64
    for k in ('mean', 'sd', 'pos'):
        np.testing.assert_allclose(got[k].numpy(), want[k], rtol=2.0 ** -23, atol=1e-12, err_msg=k)
    for k in ('chain_ape', 'chain_abs'):
        np.testing.assert_allclose(got[k].numpy(), want[k], rtol=1e-12, atol=1e-15, err_msg=k)
    assert (got['dropped'].numpy() == 0).all() and (got['chain_kept'].numpy() == case.S * case.N).all()
    if case.C == 1:                                                         # [S, d] is one chain
        one = M.sensitivities_dense(_spec(case), torch.from_numpy(theta.copy()), torch.from_numpy(X.copy()))
        np.testing.assert_allclose(one['chain_ape'].numpy(), want['chain_ape'], rtol=1e-12, atol=1e-15)


def test_dense_drop_rule():
    """A NaN weight drops its draw on every row, an inf input drops its row for every draw; the rest is as without them."""
    from mile_amd import metrics as M
    case = SC.BY_ID['1-stock']
    ospec, _, theta, X = SC.problem(case.id)
    theta, X = theta.copy(), X.copy()
    theta[2, O.param_slices(ospec)[1]['kernel'][0]] = np.nan
    X[5, 3] = np.inf
    got = M.sensitivities_dense(_spec(case), torch.from_numpy(theta), torch.from_numpy(X))
    want = R.sensitivities(ospec, theta, X, 1)
    dropped = got['dropped'].numpy()
    assert (dropped == want['dropped']).all() and dropped[5] == 7 and (np.delete(dropped, 5) == 1).all()
    assert int(got['chain_kept'][0]) == 6 * 69 == int(want['chain_kept'][0])
    assert np.isnan(got['mean'][5].numpy()).all() and np.isnan(got['sd'][5].numpy()).all() and np.isnan(got['pos'][5].numpy()).all()
    rows = np.arange(case.N) != 5
    for k in ('mean', 'sd', 'pos'):
        np.testing.assert_allclose(got[k].numpy()[rows], want[k][rows], rtol=2.0 ** -23, atol=1e-12, err_msg=k)
    clean = R.sensitivities(ospec, np.delete(theta, 2, axis=0), X[rows], 1)
    np.testing.assert_allclose(got['chain_ape'].numpy(), clean['chain_ape'], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got['mean'].numpy()[rows], clean['mean'], rtol=2.0 ** -23, atol=1e-12)


def test_summary_of_a_hand_made_result():
    from mile_amd import metrics as M
    # two chains, P = 1, F = 3; four rows, one of them with nothing kept
    res = {'chain_ape': np.array([[[1.0, -2.0, 0.5]], [[3.0, -2.0, -0.5]]]), 'chain_abs': np.array([[[1.0, 2.0, 4.0]], [[3.0, 2.0, 6.0]]]),
           'chain_kept': np.array([8, 8]),
           'pos': np.array([[[1.0, 0.0, 0.5]], [[0.96, 0.04, 0.5]], [[0.5, 0.06, 0.95]], [[np.nan, np.nan, np.nan]]], dtype=np.float32),
           'mean': np.zeros((4, 1, 3), np.float32), 'sd': np.zeros((4, 1, 3), np.float32), 'dropped': np.array([0, 0, 0, 4], np.int32)}
    s = M.sensitivity_summary(res, feature_names=['a', 'b', 'c'])
    assert s['ape'] == [[2.0, -2.0, 0.0]] and s['importance'] == [[2.0, 2.0, 5.0]]
    np.testing.assert_allclose(s['chain_sd'], [[np.sqrt(2.0), 0.0, np.sqrt(0.5)]], rtol=1e-15)
    np.testing.assert_allclose(s['decided'], [[2 / 3, 2 / 3, 1 / 3]], rtol=1e-15)
    assert s['ranking'] == [[2, 0, 1]] and s['ranked_names'] == [['c', 'a', 'b']]        # ties keep the feature order
    assert s['n_chains'] == 2 and s['n_rows'] == 3
    one = M.sensitivity_summary({k: (v[:1] if k.startswith('chain') else v) for k, v in res.items()})
    assert one['chain_sd'] == [[0.0, 0.0, 0.0]] and one['ape'] == [[1.0, -2.0, 0.5]] and 'ranked_names' not in one
    with pytest.raises(ValueError):
        M.sensitivity_summary(res, feature_names=['a'])


def test_linear_net_has_its_weights_for_jacobian():
    """Case 8, no hidden layer: J[s, n, o, f] == W_0[s][f][o] on every row, bit for bit in both precisions."""
    ospec, _, theta, X = SC.problem('8-linear')
    ref = SC.reference('8-linear')
    W0 = O.unravel(ospec, theta)[0][0]                                           # [M, F, O]
    want = np.broadcast_to(np.swapaxes(W0, 1, 2)[:, None], ref['J32'].shape)
    assert ref['J32'].dtype == np.float32 and (ref['J32'] == want).all() and (ref['J64'] == want.astype(np.float64)).all()


@pytest.mark.parametrize('cid', [c.id for c in SC.RELU_CASES])
def test_relu_condition_leaves_few_rows_out(cid):
    """The rows that the device test leaves out of a ReLU case's per-row comparison: at most 5 % of the case's rows."""
    case = SC.BY_ID[cid]
    near = SC.reference(cid)['near']
    print(f'{cid}: {near.sum()} of {case.N} rows have a hidden pre-activation within 4e-6 of 0')
    assert near.shape == (case.N,) and near.sum() <= 0.05 * case.N


@pytest.mark.parametrize('cid', [c.id for c in SC.CASES])
def test_case_inputs_are_well_chosen(cid):
    """What the device test asks of a case before it compares anything: Jacobians of a size worth comparing, and a float32
    restatement within 1e-3 of each family's largest value."""
    case = SC.BY_ID[cid]
    ref = SC.reference(cid)
    keep = ~ref['near']
    s64 = R.statistics(ref['raw64'][:, keep], ref['J64'][:, keep], case.C)
    s32 = R.statistics(ref['raw32'][:, keep], ref['J32'][:, keep], case.C)
    assert np.abs(ref['J64']).max() >= 1e-3
    for k in ('mean', 'sd', 'chain_ape', 'chain_abs'):
        e32, top = np.abs(s32[k] - s64[k]).max(), np.abs(s64[k]).max()
        print(f'{cid} {k}: float32 restatement {e32:.3e}, max|ref| = {top:.3e}')
        assert e32 <= 1e-3 * top, (cid, k, e32, top)
