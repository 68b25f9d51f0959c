"""The fp64 restatement of mile_lppd_stream (tests/lppd_ref.py) against metrics.lppd / metrics.running_lppd where those are
finite, what it gives where the literal exp / cumsum / log form underflows, the NaN rule, the default curve grid and the
evaluate.py option (function level: evaluate.py itself needs the device)."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from mile_amd import metrics as M
from tests.lppd_ref import ref_lppd_stream


def _pw(C, S, N, seed, lo=-20.0, hi=0.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=(C, S, N))


@pytest.mark.parametrize('C,S,N', [(1, 1, 1), (3, 7, 13), (4, 12, 5)])
def test_restatement_matches_the_literal_forms_where_they_are_finite(C, S, N):
    pw = _pw(C, S, N, seed=C + S)
    ref = ref_lppd_stream(pw, range(1, S + 1))
    t = torch.from_numpy(pw)
    np.testing.assert_allclose(ref['lppd'], float(M.lppd(t)), rtol=1e-10)
    np.testing.assert_allclose(ref['run_chain'], M.running_lppd(t).numpy(), rtol=1e-10)
    np.testing.assert_allclose(ref['run_ens'], [float(M.lppd(t[:, :k])) for k in range(1, S + 1)], rtol=1e-10)
    np.testing.assert_allclose(ref['chain_lppd'], [float(M.lppd(t[c:c + 1])) for c in range(C)], rtol=1e-10)
    assert ref['run_ens'][-1] == ref['lppd'] == ref['row_lppd'].mean() and not ref['dropped'].any()
    sparse = ref_lppd_stream(pw, [1, S] if S > 1 else [1])
    assert sparse['run_chain'][-1] == ref['run_chain'][-1] and sparse['run_ens'][0] == ref['run_ens'][0]


def test_the_literal_fp32_form_underflows_and_the_restatement_does_not():
    """Rows at -200 in the early draws: exp(l) = 0 in fp32, so log(cumsum / k) = -inf until a better draw arrives."""
    C, S, N = 3, 9, 11
    pw = _pw(C, S, N, seed=1)
    pw[:, :4, ::3] = -200.0 + _pw(C, 4, len(range(0, N, 3)), seed=2, lo=-5.0, hi=0.0)
    lit_terms = torch.log(torch.cumsum(torch.exp(torch.from_numpy(pw.astype(np.float32))), dim=1)
                          / torch.arange(1, S + 1, dtype=torch.float32)[None, :, None])           # running_lppd before its means
    lit = M.running_lppd(torch.from_numpy(pw.astype(np.float32))).numpy()
    assert np.isneginf(lit[:4]).all() and np.isfinite(lit[4:]).all()
    assert torch.isneginf(lit_terms).any()
    ref = ref_lppd_stream(pw, range(1, S + 1))
    assert all(np.isfinite(ref[k]).all() for k in ('run_chain', 'run_ens', 'chain_lppd', 'row_lppd', 'lppd'))
    np.testing.assert_allclose(ref['run_chain'][4:], lit[4:], rtol=2e-6)          # (fp32 literal form against fp64)
    assert ref['run_chain'][0] < -50.0                                             # the early points are low, not -inf


def test_nan_rule_of_the_restatement():
    C, S, N = 3, 5, 4
    pw = _pw(C, S, N, seed=5)
    pw[1, 2, :] = np.nan                                       # one draw of chain 1 on every row
    ref = ref_lppd_stream(pw, range(1, S + 1))
    assert ref['dropped'].tolist() == [0, N, 0]
    without = ref_lppd_stream(np.delete(pw[1:2], 2, axis=1), range(1, S))
    np.testing.assert_allclose(ref['chain_lppd'][1], without['chain_lppd'][0], rtol=1e-14)
    full = ref_lppd_stream(_pw(C, S, N, seed=5), range(1, S + 1))
    assert ref['chain_lppd'][0] == full['chain_lppd'][0] and ref['chain_lppd'][2] == full['chain_lppd'][2]
    pw[1] = np.nan                                             # a chain without a draw
    ref = ref_lppd_stream(pw, range(1, S + 1))
    assert np.isnan(ref['chain_lppd'][1]) and np.isnan(ref['run_chain']).all()
    assert np.isfinite(ref['run_ens']).all() and np.isfinite(ref['row_lppd']).all()
    two = ref_lppd_stream(pw[[0, 2]], range(1, S + 1))
    np.testing.assert_allclose(ref['run_ens'], two['run_ens'], rtol=1e-14)
    pw[0, :, 1] = -np.inf                                      # -inf takes part: it adds 0 and is counted
    ref = ref_lppd_stream(pw, [S])
    assert ref['dropped'].tolist() == [0, S * N, 0] and np.isneginf(ref['chain_lppd'][0]) and np.isfinite(ref['lppd'])


@pytest.mark.parametrize('S,n', [(1, 64), (2, 64), (64, 64), (65, 64), (1000, 64), (1000, 16), (10 ** 6, 64), (7, 2), (50, 1)])
def test_curve_points(S, n):
    pts = M.curve_points(S, n)
    assert len(pts) == min(S, n) and pts[-1] == S and all(isinstance(k, int) for k in pts)
    assert all(b > a for a, b in zip(pts, pts[1:])) and pts[0] >= 1
    if S <= n:
        assert pts == list(range(1, S + 1))
    elif n > 1:
        assert pts[0] == 1
        if S >= 100 * n:                                       # geometric: the later gaps grow
            gaps = np.diff(pts[n // 2:])
            assert (np.diff(gaps) >= 0).all()


def test_curve_points_default_and_refusal():
    assert M.curve_points(1000) == M.curve_points(1000, 64) and len(M.curve_points(1000)) == 64
    with pytest.raises(ValueError):
        M.curve_points(0)


def test_evaluate_running_option():
    import evaluate as EV
    ap = EV.build_parser()
    assert ap.parse_args(['-e', 'x']).running is None                          # opt-in
    assert ap.parse_args(['-e', 'x', '--running']).running == 64
    assert ap.parse_args(['-e', 'x', '--running', '16']).running == 16
    pw = _pw(3, 6, 5, seed=9)
    pts = M.curve_points(6, 4)
    ref = ref_lppd_stream(pw, pts)
    res = {k: torch.as_tensor(v) for k, v in ref.items()}
    res['curve_points'] = torch.tensor(pts, dtype=torch.int32)
    keys, arrays = EV.running_metrics(res)
    assert sorted(arrays) == ['chain_lppd', 'curve_points', 'dropped', 'row_lppd', 'run_chain', 'run_ens']
    assert all(k.startswith('running_') for k in keys)
    assert keys['running_points'] == 4 and keys['running_lppd'] == ref['lppd'] == keys['running_ens_last']
    assert keys['running_per_chain_lppd'] == ref['chain_lppd'].tolist() and keys['running_dropped'] == 0
    assert keys['running_chain_first'] == ref['run_chain'][0] and keys['running_ens_first'] == ref['run_ens'][0]
