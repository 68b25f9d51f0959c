"""The host side of the chain-weighted mixture (no GPU): the NumPy fp64 reference of tests/wquantile_ref.py tied to the
committed reference of the equal-weight mixture (tests/quantile_ref.py) by replication, the torch forms of metrics.py against
it, the exact composition of per-chain moments and class probabilities, the weight checks, the C ABI (prototypes, and the
refusals, every one decided before anything touches a device), predict.py's refusal of a vector of the wrong length and the
stacked keys of evaluate.py.

The replication anchor.  For rational weights w_c = k_c / sum k and chains without a dropped draw, the weighted mixture IS
the equal-weight mixture of the draws with chain c repeated k_c times: the same function F, summed in another order.  fp64
sums of <= 200 terms in [0, 1] differ by <= 200 * 2^-53 = 2e-14 in F; a quantile moves by that over the density, far below
1e-10 sd_n wherever the density is not < 2e-4 / sd_n, and the levels used keep away from that.  Hence: quantiles within
1e-10 sd_n, PIT within 1e-12.  Measured: max |dq| / sd_n = 2.5e-14, max |dpit| = 7e-16."""
from __future__ import annotations

import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from mile_amd import metrics as M
from tests import quantile_ref as QR
from tests import wquantile_ref as WR

ROOT = Path(__file__).resolve().parents[1]
LEVELS = [0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975]


def _raw(Cn, S, N, seed):
    """Chains that do not mix: every chain has its own offset, of the order of the spread within it."""
    rng = np.random.default_rng(seed)
    centre, spread = rng.standard_normal(N) * 3.0, np.exp(rng.uniform(-3.0, 1.0, N))
    mu = centre + spread * rng.standard_normal((Cn, S, N)) + 1.5 * spread * rng.standard_normal((Cn, 1, N))
    ls = rng.uniform(-2.0, 1.0, N) + 0.5 * rng.standard_normal((Cn, S, N))
    raw = np.stack([mu, ls], axis=-1).astype(np.float32)
    y = (raw[rng.integers(0, Cn, N), rng.integers(0, S, N), np.arange(N), 0] + rng.standard_normal(N)).astype(np.float32)
    return raw, y


def _replicated(raw, k):
    """[sum_c k_c * S, N, 2]: chain c's draws k_c times."""
    return np.concatenate([raw[c] for c in range(raw.shape[0]) for _ in range(k[c])], axis=0)


@pytest.mark.parametrize('k', [(1, 0, 3), (2, 5, 1), (1, 1, 1), (0, 0, 1)])
def test_replication_anchor(k):
    raw, y = _raw(3, 9, 11, 1)
    w = np.array(k, dtype=np.float64) / sum(k)
    rep = _replicated(raw, k)
    sd = QR.mixture_sd(rep)
    dq = np.abs(WR.quantiles(raw, w, LEVELS) - QR.quantiles(rep, LEVELS)) / sd[:, None]
    dp = np.abs(WR.pit(raw, w, y) - QR.pit(rep, y))
    print(f'k = {k}: max |dq| / sd = {dq.max():.2e}, max |dpit| = {dp.max():.2e}')
    assert dq.max() <= 1e-10 and dp.max() <= 1e-12
    np.testing.assert_allclose(WR.mixture_sd(raw, w), sd, rtol=1e-12)
    if len(set(k)) == 1:                                           # w = 1 / C: the pooled reference on the draws as they are
        pooled = raw.reshape(-1, *raw.shape[2:])
        assert (np.abs(WR.quantiles(raw, w, LEVELS) - QR.quantiles(pooled, LEVELS)) <= 1e-10 * sd[:, None]).all()
        assert np.abs(WR.pit(raw, w, y) - QR.pit(pooled, y)).max() <= 1e-12


def _poisoned():
    """Chain 1 all NaN on every row (zero weight below), chain 0 with single draws dropped, chain 2 empty on row 4."""
    raw, y = _raw(3, 9, 11, 2)
    raw[1] = np.nan
    raw[0, 2, 0, 0] = np.nan
    raw[0, 3, 0, 1] = np.inf
    raw[2, 5, 1, 0] = -np.inf
    raw[2, :, 4, 1] = np.nan
    return raw, y


def test_reference_leave_out_rules():
    raw, y = _poisoned()
    w = np.array([0.25, 0.0, 0.75])
    q, p = WR.quantiles(raw, w, LEVELS), WR.pit(raw, w, y)
    bad = np.arange(11) == 4
    assert np.isnan(q[bad]).all() and np.isnan(p[bad]).all() and np.isfinite(q[~bad]).all() and np.isfinite(p[~bad]).all()
    want = np.zeros((3, 11), dtype=np.int32)
    want[1], want[0, 0], want[2, 1], want[2, 4] = 9, 2, 1, 9
    assert np.array_equal(WR.dropped(raw), want)
    assert np.abs(WR.cdf(raw, w, q)[~bad] - np.asarray(LEVELS)).max() <= 1e-12
    # weight on the all-NaN chain: every row NaN
    assert np.isnan(WR.quantiles(raw, [0.2, 0.3, 0.5], LEVELS)).all() and np.isnan(WR.pit(raw, [0.2, 0.3, 0.5], y)).all()


@pytest.mark.parametrize('w', [(0.25, 0.0, 0.75), (1 / 3, 1 / 3, 1 / 3), (0.0, 0.0, 1.0), (0.2, 0.3, 0.5)])
def test_torch_forms_are_the_reference(w):
    raw, y = _poisoned()
    if w[1] > 0:
        raw[1] = _raw(3, 9, 11, 3)[0][1]
    rt = torch.from_numpy(raw)
    q, dropped = M.weighted_mixture_quantiles(rt, w, LEVELS, return_dropped=True)
    p = M.weighted_mixture_pit(rt, w, torch.from_numpy(y))
    assert q.dtype == p.dtype == torch.float64 and dropped.dtype == torch.int32
    ref_q, ref_p, sd = WR.quantiles(raw, w, LEVELS), WR.pit(raw, w, y), WR.mixture_sd(raw, w)
    assert np.array_equal(np.isnan(q.numpy()), np.isnan(ref_q)) and np.array_equal(np.isnan(p.numpy()), np.isnan(ref_p))
    fin = np.isfinite(ref_p)
    assert fin.sum() == 10
    assert (np.abs(q.numpy() - ref_q)[fin] <= 1e-10 * sd[fin, None]).all()
    assert np.abs(p.numpy() - ref_p)[fin].max() <= 1e-12
    assert np.array_equal(dropped.numpy(), WR.dropped(raw))
    assert (np.diff(q.numpy()[fin], axis=1) >= 0).all()


def _chain_moments(raw, task):
    """per-chain predictive_moments in fp64 and the kept counts."""
    mom = torch.stack([M.predictive_moments(torch.from_numpy(raw[c]).double(), task) for c in range(raw.shape[0])])
    kept = torch.from_numpy(np.isfinite(raw).all(axis=-1).sum(axis=1).astype(np.int32))
    return mom, kept


def test_weighted_moments_are_the_moments_of_the_replicated_draws():
    raw, _ = _raw(4, 6, 9, 4)
    raw[3, :, 2, 0] = np.nan                                        # chain 3: K_c = 0 on row 2
    raw[0, 1, 5, 1] = np.inf                                        # chain 0 drops one draw on row 5
    k = (2, 0, 3, 1)
    w = np.array(k, dtype=np.float64) / sum(k)
    mom, kept = _chain_moments(raw, 'regr')
    got = M.weighted_moments(mom, kept, w, 'regr').numpy()
    assert got.shape == (9, 3) and np.isnan(got[2]).all() and np.isfinite(np.delete(got, 2, axis=0)).all()
    for n in range(9):
        if n == 2:
            continue
        mu, s2, wt = [], [], []
        for c in range(4):
            ok = np.isfinite(raw[c, :, n]).all(axis=-1)
            mu.append(raw[c, ok, n, 0].astype(np.float64))
            s2.append(np.clip(np.exp(raw[c, ok, n, 1].astype(np.float64)), 1e-6, 1e6) ** 2)
            wt.append(np.full(ok.sum(), w[c] / ok.sum()))
        mu, s2, wt = np.concatenate(mu), np.concatenate(s2), np.concatenate(wt)
        mean = (wt * mu).sum()
        want = np.array([mean, (wt * (mu - mean) ** 2).sum(), (wt * s2).sum()])
        np.testing.assert_allclose(got[n], want, rtol=1e-11, atol=1e-13)
    # without a dropped draw: NumPy's moments of the draws with chain c repeated k_c times
    clean, _ = _raw(4, 6, 9, 5)
    rep = _replicated(clean, k).astype(np.float64)
    mom, kept = _chain_moments(clean, 'regr')
    got = M.weighted_moments(mom, kept, w, 'regr').numpy()
    want = np.stack([rep[..., 0].mean(axis=0), rep[..., 0].var(axis=0), (np.exp(rep[..., 1]) ** 2).mean(axis=0)], axis=-1)
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-13)
    # a zero-weight chain with nothing kept poisons nothing
    clean[1] = np.nan
    mom, kept = _chain_moments(clean, 'regr')
    np.testing.assert_allclose(M.weighted_moments(mom, kept, w, 'regr').numpy(), want, rtol=1e-11, atol=1e-13)


def test_weighted_class_probs_and_sets():
    rng = np.random.default_rng(6)
    Cn, S, N, K = 3, 5, 12, 4
    logits = (2.0 * rng.standard_normal((Cn, S, N, K))).astype(np.float32)
    logits[2, :, 7] = np.nan                                        # chain 2: nothing kept on row 7
    logits[0, 1, 3, 2] = np.inf                                     # chain 0 drops a draw on row 3
    y = rng.integers(0, K, N)
    w = np.array([0.5, 0.0, 0.5])
    mom, kept = _chain_moments(logits, 'classification')
    P, k = M.weighted_class_probs(mom[..., :K], kept, w)
    ok = np.isfinite(logits).all(axis=-1)
    lg = np.where(ok[..., None], logits, 0.0).astype(np.float64)
    sm = np.exp(lg - lg.max(axis=-1, keepdims=True))
    sm = sm / sm.sum(axis=-1, keepdims=True) * ok[..., None]
    with np.errstate(invalid='ignore', divide='ignore'):
        Pc = sm.sum(axis=1) / ok.sum(axis=1)[..., None]                 # [C, N, K]
    want = 0.5 * Pc[0] + 0.5 * Pc[2]
    assert np.isnan(P.numpy()[7]).all() and k[7] == 0
    rows = np.arange(N) != 7
    np.testing.assert_allclose(P.numpy()[rows], want[rows], rtol=1e-12, atol=1e-15)
    assert k.tolist() == [0 if n == 7 else (9 if n == 3 else 10) for n in range(N)]
    # entropy and mutual information of the weighted mixture from the chains' own
    got = M.weighted_moments(mom, kept, w, 'classification').numpy()
    with np.errstate(invalid='ignore', divide='ignore'):
        h = -(want * np.log(want)).sum(axis=-1)
        hd = -np.where(sm > 0, sm * np.log(np.where(sm > 0, sm, 1.0)), 0.0).sum(axis=-1)        # [C, S, N]
        hc = hd.sum(axis=1) / ok.sum(axis=1)
    mi = h - (0.5 * hc[0] + 0.5 * hc[2])
    np.testing.assert_allclose(got[rows, :K], want[rows], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got[rows, K], h[rows], rtol=1e-11)
    np.testing.assert_allclose(got[rows, K + 1], mi[rows], rtol=1e-9, atol=1e-12)
    assert np.isnan(got[7]).all()
    # the sets of P, directly: classes by descending probability, the first whose cumulative sum reaches the level
    cov = [0.5, 0.9]
    dec = M.calibration_decide(P[None], k[None], torch.from_numpy(y), cov)
    for n in np.flatnonzero(rows):
        order = np.argsort(-want[n], kind='stable')
        assert dec['order'][n].tolist() == order.tolist()
        cum = np.cumsum(want[n][order])
        assert dec['set_size'][n].tolist() == [int(np.argmax(cum >= c)) + 1 if (cum >= c).any() else K for c in cov]
        assert int(dec['rank'][n]) == order.tolist().index(int(y[n])) + 1
    assert dec['set_size'][7].tolist() == [0, 0] and int(dec['rank'][7]) == 0
    assert float(dec['totals'][0, 0]) == N - 1


def test_chain_weights_refusals():
    assert M.chain_weights([0.5, 0.25, 0.25 + 5e-10], 3).dtype == torch.float64
    assert M.chain_weights(np.array([1.0]), 1).tolist() == [1.0]
    for w in ([0.5, 0.5], [0.25] * 4, [[0.5, 0.25, 0.25]], [0.5, 0.75, -0.25], [0.5, float('nan'), 0.5], [float('inf'), 0.0, 0.0],
              [0.5, 0.25, 0.25 + 1e-8], [0.0, 0.0, 0.0]):
        with pytest.raises(ValueError):
            M.chain_weights(w, 3)
    raw, y = _raw(3, 4, 5, 7)
    with pytest.raises(ValueError):
        M.weighted_mixture_quantiles(torch.from_numpy(raw), [0.5, 0.5], LEVELS)
    with pytest.raises(ValueError):
        M.weighted_mixture_quantiles(torch.from_numpy(raw[0]), [1.0], LEVELS)
    with pytest.raises(ValueError):
        M.weighted_mixture_quantiles(torch.from_numpy(raw), [0.5, 0.25, 0.25], [0.0, 0.5])


# ---------------------------------------------------------------- C ABI -------------------------
def test_library_exports_the_weighted_symbols_under_abi_10():
    from mile_amd import _lib
    from mile_amd._build import build_library
    build_library()
    lib = _lib.load_library()
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    want = {'mile_mixture_quantiles_weighted': (i32, [p, i32, i64, i64, p, p, i32, p, p, p, p, p]),
            'mile_predict_quantiles_weighted': (i32, [p, p, i32, i64, p, i64, p, p, i32, p, p, p, p, i64, i64, p]),
            'mile_predict_quantiles_weighted_workspace': (i64, [p, i32, i64, i64])}
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == sig[1]
    assert lib.mile_abi_version() == _lib.ABI_VERSION == 10
    header = ' '.join((ROOT / 'include' / 'mile_hip.h').read_text().split())
    assert ('int32_t mile_mixture_quantiles_weighted(const float *raw, int32_t C, int64_t S, int64_t N, const double *weights, '
            'const double *levels, int32_t Q, const float *y, float *quant, float *pit, int32_t *dropped /* [C, N] */, '
            'void *stream);') in header
    assert ('int32_t mile_predict_quantiles_weighted(mile_sampler *s, const float *theta /* [C*S, d] */, int32_t C, int64_t S, '
            'const void *X, int64_t N, const double *weights, const double *levels, int32_t Q, const float *y, float *quant, '
            'float *pit, int32_t *dropped, int64_t max_draws_per_pass, int64_t max_rows_per_tile, void *stream);') in header
    assert 'int64_t mile_predict_quantiles_weighted_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N);' in header


def _doubles(v):
    return (C.c_double * len(v))(*v)


BAD = [('null raw', dict(raw=None), 'null raw'), ('C = 0', dict(Cn=0), 'C out of range (1 .. 1024)'), ('C = 1025', dict(Cn=1025), 'C out of range'),
       ('S = 0', dict(S=0), 'C * S out of range'), ('C * S = 2^31', dict(Cn=2, S=1 << 30), 'C * S out of range'),
       ('N = 0', dict(N=0), 'N out of range'), ('N = 2^30', dict(N=1 << 30), 'N out of range'),
       ('null weights', dict(w=None), 'null weights'), ('negative weight', dict(w=_doubles([0.5, 0.75, -0.25])), 'finite and >= 0'),
       ('nan weight', dict(w=_doubles([0.5, float('nan'), 0.5])), 'finite and >= 0'),
       ('inf weight', dict(w=_doubles([float('inf'), 0.0, 0.0])), 'finite and >= 0'),
       ('sum off by 1e-8', dict(w=_doubles([0.5, 0.25, 0.25 + 1e-8])), 'sum to 1'),
       ('null levels', dict(lev=None), 'null levels'), ('Q = 0', dict(Q=0), 'Q out of range'), ('Q = 33', dict(Q=33), 'Q out of range'),
       ('level 0', dict(lev=_doubles([0.0, 0.5])), 'strictly inside'), ('levels not increasing', dict(lev=_doubles([0.5, 0.5])), 'strictly increasing'),
       ('pit without y', dict(y=None), 'PIT needs y'), ('no output', dict(quant=None, pit=None), 'neither quantiles nor PIT')]


def test_mixture_quantiles_weighted_refuses_bad_arguments_without_a_gpu():
    from mile_amd import _lib
    lib = _lib.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(raw=p, Cn=3, S=8, N=4, w=_doubles([0.5, 0.25, 0.25]), lev=_doubles([0.25, 0.75]), Q=2, y=p, quant=p, pit=p, dropped=p):
        return lib.mile_mixture_quantiles_weighted(raw, Cn, S, N, w, lev, Q, y, quant, pit, dropped, None)
    for tag, kw, text in BAD:
        assert call(**kw) == -1, tag
        msg = lib.mile_last_error().decode()
        assert 'mile_mixture_quantiles_weighted' in msg and text in msg, (tag, msg)
    assert lib.mile_predict_quantiles_weighted_workspace(None, 3, 8, 4) == -1
    assert lib.mile_predict_quantiles_weighted(None, p, 3, 8, p, 4, _doubles([0.5, 0.25, 0.25]), _doubles([0.5]), 1, p, p, p, p, 0, 0, None) == -1


# ---------------------------------------------------------------- predict.py --------------------
def test_predict_refuses_a_weight_vector_of_another_length(tmp_path):
    sys.path.insert(0, str(ROOT))
    try:
        import predict
    finally:
        sys.path.remove(str(ROOT))
    np.savez(tmp_path / 'stacking.npz', weights=np.array([0.5, 0.25, 0.25]))
    np.save(tmp_path / 'w.npy', np.array([0.75, 0.25]))
    (tmp_path / 'w.txt').write_text('0.5\n0.5\n')
    np.savez(tmp_path / 'other.npz', w=np.array([1.0]))
    np.testing.assert_array_equal(predict.read_weights('stacking', tmp_path, 3), [0.5, 0.25, 0.25])
    np.testing.assert_array_equal(predict.read_weights(tmp_path / 'w.npy', tmp_path, 2), [0.75, 0.25])
    np.testing.assert_array_equal(predict.read_weights(tmp_path / 'w.txt', tmp_path, 2), [0.5, 0.5])
    with pytest.raises(SystemExit, match='holds 3 weights, 2 chains are loaded'):      # --drop-nonfinite took a chain out
        predict.read_weights('stacking', tmp_path, 2)
    with pytest.raises(SystemExit, match='holds 2 weights, 4 chains'):
        predict.read_weights(tmp_path / 'w.npy', tmp_path, 4)
    with pytest.raises(SystemExit, match='no array "weights"'):
        predict.read_weights(tmp_path / 'other.npz', tmp_path, 1)
    with pytest.raises(SystemExit, match='does not exist'):
        predict.read_weights('stacking', tmp_path / 'nowhere', 3)
    np.save(tmp_path / 'neg.npy', np.array([1.5, -0.5]))
    with pytest.raises(SystemExit, match='finite and >= 0'):
        predict.read_weights(tmp_path / 'neg.npy', tmp_path, 2)
    assert '--weights' in subprocess.run([sys.executable, str(ROOT / 'predict.py'), '--help'], capture_output=True, text=True, check=True).stdout


# ---------------------------------------------------------------- evaluate.py -------------------
def test_stacked_keys_of_evaluate():
    sys.path.insert(0, str(ROOT))
    try:
        import evaluate
    finally:
        sys.path.remove(str(ROOT))
    # --calibration: P = sum_c w_c P_c scored directly
    rng = np.random.default_rng(8)
    Cn, S, N, K = 3, 6, 40, 4
    logits = torch.from_numpy((2.0 * rng.standard_normal((Cn, S, N, K))).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, K, N))
    w = np.array([0.6, 0.0, 0.4])
    res = M.classification_calibration(logits, y, coverages=(0.5, 0.9), n_bins=5)
    keys = evaluate.stacked_calibration_metrics(res, w, y, 5)
    assert sorted(keys) == ['calibration_stacked_accuracy', 'calibration_stacked_brier', 'calibration_stacked_ece', 'calibration_stacked_nll']
    P = (0.6 * torch.softmax(logits[0].double(), -1).mean(0) + 0.4 * torch.softmax(logits[2].double(), -1).mean(0)).numpy()
    yy = y.numpy()
    assert keys['calibration_stacked_nll'] == pytest.approx(float(-np.log(P[np.arange(N), yy]).mean()), rel=1e-12)
    assert keys['calibration_stacked_brier'] == pytest.approx(float(((P - np.eye(K)[yy]) ** 2).sum(axis=1).mean()), rel=1e-12)
    assert keys['calibration_stacked_accuracy'] == pytest.approx(float((P.argmax(axis=1) == yy).mean()), rel=1e-12)
    conf, hit = P.max(axis=1), P.argmax(axis=1) == yy
    b = np.minimum(np.floor(conf * 5).astype(int), 4)
    ece = sum(abs(hit[b == k].sum() - conf[b == k].sum()) for k in range(5)) / N
    assert keys['calibration_stacked_ece'] == pytest.approx(float(ece), rel=1e-10)
    # one-hot weights: the chain's own figures of the calibration result
    own = M.calibration_summary({k: res[k] for k in ('totals', 'bins', 'coverages')})[1]
    hot = evaluate.stacked_calibration_metrics(res, [0.0, 1.0, 0.0], y, 5)
    assert hot['calibration_stacked_nll'] == pytest.approx(own['nll'], rel=1e-12) and hot['calibration_stacked_ece'] == pytest.approx(own['ece'], rel=1e-10)
    # --intervals: the keys of interval_metrics under their stacked names
    raw, yr = _raw(3, 9, 25, 9)
    cov = [0.5, 0.9]
    levels = M.interval_levels(cov)
    q = M.weighted_mixture_quantiles(torch.from_numpy(raw), w, levels)
    pit = M.weighted_mixture_pit(torch.from_numpy(raw), w, torch.from_numpy(yr))
    keys, arrays = evaluate.stacked_interval_metrics(q, pit, levels, cov)
    assert sorted(keys) == ['intervals_stacked_cal_error', 'intervals_stacked_coverage_0.5', 'intervals_stacked_coverage_0.9',
                            'intervals_stacked_width_0.5', 'intervals_stacked_width_0.9']
    assert sorted(arrays) == ['pit_stacked', 'quantiles_stacked'] and arrays['quantiles_stacked'].shape == (25, 4)
    inside = (q[:, 0].numpy() <= yr) & (yr <= q[:, 3].numpy())
    assert keys['intervals_stacked_coverage_0.9'] == pytest.approx(float(inside.mean()), abs=1e-12)
    np.testing.assert_allclose(evaluate.stacked_weights([0.5, -1e-17, 0.5 + 1e-12]), [0.5, 0.0, 0.5], atol=1e-12)
