"""metrics.predictive_moments -- the torch restatement of mile_predict_moments -- against a direct fp64 NumPy computation,
its shifted variance under cancellation, the law of total variance, and the keys evaluate.py --moments writes (function
level: evaluate.py itself needs the device)."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from mile_amd import metrics as M


def _xlogx(p):
    return np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)


def ref_moments(out, task):
    """Direct fp64 NumPy: out [S, N, O] (all finite) -> [N, W]."""
    out = np.asarray(out, dtype=np.float64)
    if task == 'regr':
        mu, sig = out[..., 0], np.clip(np.exp(out[..., 1]), 1e-6, 1e6)
        return np.stack([mu.mean(axis=0), mu.var(axis=0), (sig ** 2).mean(axis=0)], axis=-1)
    z = out - out.max(axis=-1, keepdims=True)
    p = np.exp(z) / np.exp(z).sum(axis=-1, keepdims=True)
    pm = p.mean(axis=0)
    h = -_xlogx(pm).sum(axis=-1)
    mi = np.maximum(h - (-_xlogx(p).sum(axis=-1)).mean(axis=0), 0.0)
    return np.concatenate([pm, h[:, None], mi[:, None]], axis=-1)


@pytest.mark.parametrize('S', [1, 2, 9])
@pytest.mark.parametrize('task,O', [('regr', 2), ('classification', 5)])
def test_restatement_matches_fp64_numpy(task, O, S):
    rng = np.random.default_rng(S + O)
    out = rng.standard_normal((S, 13, O)) * (0.7 if task == 'regr' else 2.0)
    got = M.predictive_moments(torch.from_numpy(out), task).numpy()
    ref = ref_moments(out, task)
    assert got.shape == (13, 3 if task == 'regr' else O + 2)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-14)
    if S == 1:                                                     # one draw: no spread between draws, exactly
        assert (got[:, 1] == 0).all() if task == 'regr' else (got[:, O + 1] == 0).all()
    got32 = M.predictive_moments(torch.from_numpy(out.astype(np.float32)), task)
    assert got32.dtype == torch.float32
    np.testing.assert_allclose(got32.numpy(), ref, rtol=2e-5, atol=2e-6)
    if S == 1:
        assert (got32[:, 1] == 0).all() if task == 'regr' else (got32[:, O + 1] == 0).all()


def test_leading_axes_are_draw_axes():
    rng = np.random.default_rng(0)
    out = rng.standard_normal((3, 4, 7, 2))
    a = M.predictive_moments(torch.from_numpy(out), 'regr')
    b = M.predictive_moments(torch.from_numpy(out.reshape(12, 7, 2)), 'regr')
    assert torch.equal(a, b)


def test_fp32_variance_survives_cancellation():
    """4096 draws, mu = 100 + 1e-3 z: sum(mu^2) - sum(mu)^2 / S in fp32 has no digit of the variance left (1e4 * 6e-8 >> 1e-6);
    the shifted form keeps it."""
    rng = np.random.default_rng(1)
    mu = (100.0 + 1e-3 * rng.standard_normal((4096, 5))).astype(np.float32)
    out = np.stack([mu, np.zeros_like(mu)], axis=-1)
    ref = mu.astype(np.float64).var(axis=0)
    got = M.predictive_moments(torch.from_numpy(out), 'regr')[:, 1].numpy().astype(np.float64)
    rel = np.abs(got - ref) / ref
    print('relative error of the fp32 epistemic variance:', rel)
    assert (rel < 1e-3).all()
    naive = (mu * mu).mean(axis=0, dtype=np.float32) - mu.mean(axis=0, dtype=np.float32) ** 2
    assert (np.abs(naive.astype(np.float64) - ref) / ref > 1.0).any()      # (what the plain form gives)


def test_total_variance_is_the_mixture_variance():
    """epistemic + aleatoric = variance of the equal-weight mixture of the draws' Normals, here by sampling it in fp64."""
    rng = np.random.default_rng(2)
    S, N, R = 6, 4, 200000
    out = np.stack([rng.standard_normal((S, N)), 0.3 * rng.standard_normal((S, N))], axis=-1)
    mom = M.predictive_moments(torch.from_numpy(out), 'regr').numpy()
    y = out[..., 0][None] + np.exp(out[..., 1])[None] * rng.standard_normal((R, S, N))    # R draws of every component
    var = y.reshape(R * S, N).var(axis=0)
    se = var * np.sqrt(2.0 / (R * S)) * 3.0                 # standard error of a variance (Normal-like tails), with slack
    np.testing.assert_allclose(mom[:, 1] + mom[:, 2], var, atol=float(6 * se.max()))
    np.testing.assert_allclose(mom[:, 0], y.reshape(R * S, N).mean(axis=0), atol=float(6 * np.sqrt(var / (R * S)).max()))


def test_nonfinite_draws_leave_their_rows_only():
    rng = np.random.default_rng(3)
    out = rng.standard_normal((5, 6, 3))
    out[2, 1, 0] = np.inf
    out[4, 1, 2] = np.nan
    out[0, 3, 1] = -np.inf
    mom, dropped = M.predictive_moments(torch.from_numpy(out), 'classification', return_dropped=True)
    assert dropped.dtype == torch.int32 and dropped.tolist() == [0, 2, 0, 1, 0, 0]
    np.testing.assert_allclose(mom[1].numpy(), ref_moments(out[[0, 1, 3], 1:2], 'classification')[0], rtol=1e-12)
    np.testing.assert_allclose(mom[3].numpy(), ref_moments(out[1:, 3:4], 'classification')[0], rtol=1e-12)
    np.testing.assert_allclose(mom[0].numpy(), ref_moments(out[:, 0:1], 'classification')[0], rtol=1e-12)
    out[:, 5, 0] = np.nan                                          # no finite draw at all
    mom, dropped = M.predictive_moments(torch.from_numpy(out), 'classification', return_dropped=True)
    assert dropped[5] == 5 and torch.isnan(mom[5]).all() and torch.isfinite(mom[:5]).all()


def test_rmse_from_moments():
    mom = torch.tensor([[1.0, 0, 0], [2.0, 0, 0], [4.0, 0, 0]], dtype=torch.float64)
    y = torch.tensor([1.0, 4.0, 4.0])
    assert float(M.rmse_from_moments(y, mom)) == pytest.approx(np.sqrt(4.0 / 3.0), rel=1e-12)


def test_evaluate_moments_keys():
    import evaluate as EV
    assert EV.build_parser().parse_args(['-e', 'x']).moments is False       # opt-in
    assert EV.build_parser().parse_args(['-e', 'x', '--moments']).moments is True
    rng = np.random.default_rng(4)
    out = rng.standard_normal((7, 9, 2))
    y = rng.standard_normal(9).astype(np.float32)
    mom, dropped = M.predictive_moments(torch.from_numpy(out), 'regr', return_dropped=True)
    keys, arrays = EV.moment_metrics(mom, dropped, y, 'regr')
    assert sorted(keys) == ['moments_aleatoric_var', 'moments_dropped', 'moments_epistemic_var', 'moments_mean', 'moments_rmse']
    assert sorted(arrays) == ['aleatoric_var', 'dropped', 'epistemic_var', 'mean'] and all(a.shape == (9,) for a in arrays.values())
    ref = ref_moments(out, 'regr')
    assert keys['moments_rmse'] == pytest.approx(float(np.sqrt(((y - ref[:, 0]) ** 2).mean())), rel=1e-6)
    assert keys['moments_epistemic_var'] == pytest.approx(float(ref[:, 1].mean()), rel=1e-6)
    assert keys['moments_dropped'] == 0
    out = rng.standard_normal((7, 9, 4))
    mom, dropped = M.predictive_moments(torch.from_numpy(out), 'classification', return_dropped=True)
    keys, arrays = EV.moment_metrics(mom, dropped, rng.integers(0, 4, 9), 'class')
    assert sorted(keys) == ['moments_dropped', 'moments_entropy', 'moments_mutual_information', 'moments_probs']
    assert len(keys['moments_probs']) == 4 and sum(keys['moments_probs']) == pytest.approx(1.0, abs=1e-6)
    assert arrays['probs'].shape == (9, 4) and arrays['entropy'].shape == arrays['mutual_information'].shape == (9,)
    assert arrays['dropped'].dtype == np.int32
