"""The fp64 restatement of the calibration contract (tests/calib_ref.py) held to facts that do not come from it -- the smallest
set found by enumerating subsets, the rank found by counting, exactly calibrated bins, uniform logits -- the torch form of
mile_amd.metrics against it, and the host side of mile_calibration / mile_calibration_stream: exports, bindings, every
argument refusal through ctypes on handles created without a GPU, the CLI parsers and the CLIs' refusals."""
import ctypes as C
import itertools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from mile_amd import metrics as M
from tests import calib_ref as R
from tests.test_predict_host import _attn_pre_cspec, _fcn_cspec

ROOT = Path(__file__).resolve().parents[1]
NEW = ('mile_calibration', 'mile_calibration_stream', 'mile_calibration_stream_workspace')


# ---------------------------------------------------------------- the reference -----------------
@pytest.mark.parametrize('K', [2, 3, 4, 5])
def test_decide_against_brute_force(K):
    """Levels at the midpoints between neighbouring subset sums: no level sits within rounding of a sum, so the smallest
    covering set does not depend on the order its members are added in."""
    rng = np.random.default_rng(K)
    N = 40
    P = rng.dirichlet(np.ones(K) * 0.7, size=(2, N))
    P[0, :5] = np.round(P[0, :5] * 4) / 4                              # ties
    P[0, :5, K - 1] += 1.0 - P[0, :5].sum(axis=-1)
    y = rng.integers(0, K, N)
    kept = np.ones((2, N), dtype=np.int32)
    cov = [0.35, 0.6, 0.85, 0.97]
    d = R.decide(P, kept, y, cov, 10)
    for g in range(2):
        for n in range(N):
            p = P[g, n]
            sums = sorted({sum(p[list(s)]) for r in range(1, K + 1) for s in itertools.combinations(range(K), r)})
            if any(abs(s - c) < 1e-9 for s in sums for c in cov):
                continue
            for q, c in enumerate(cov):
                smallest = min((r for r in range(1, K + 1) for s in itertools.combinations(range(K), r) if sum(p[list(s)]) >= c - 1e-12), default=K)
                assert d['set_size'][g, n, q] == smallest, (g, n, c, p)
            rank = 1 + sum(1 for k in range(K) if p[k] > p[y[n]] or (p[k] == p[y[n]] and k < y[n]))
            assert d['rank'][g, n] == rank
            o = d['order'][g, n]
            assert sorted(o) == list(range(K)) and all(p[o[i]] > p[o[i + 1]] or (p[o[i]] == p[o[i + 1]] and o[i] < o[i + 1]) for i in range(K - 1))
    t = d['totals']
    assert (t[:, 0] == N).all() and (t[:, 1] == (d['rank'] == 1).sum(axis=1)).all()
    onehot = np.eye(K)[y]
    np.testing.assert_allclose(t[:, 2], ((P - onehot[None]) ** 2).sum(axis=(1, 2)), rtol=1e-13)
    with np.errstate(divide='ignore'):                                 # (a rounded row may give its label probability 0)
        np.testing.assert_allclose(t[:, 3], -np.log(np.take_along_axis(P, y[None, :, None], axis=2)).sum(axis=(1, 2)), rtol=1e-13)
    assert (d['bins'][..., 0].sum(axis=1) == N).all() and (d['bins'][..., 2].sum(axis=1) == t[:, 1]).all()


def test_uniform_logits():
    """All-zero logits: P is exactly 1 / K (with 2 chains of 4 draws every sum of 0.1 on the way is exact or rounds back), the
    order is by index, and at K = 10 nine sequential fp64 additions of 0.1 stay below 0.9, so the 90 % set takes all ten
    classes."""
    s = 0.0
    for _ in range(9):
        s += 0.1
    assert s < 0.9
    raw = np.zeros((2 * 4, 4, 10), dtype=np.float32)
    P, kept = R.probs(raw, 2, 4)
    assert (P == 0.1).all() and (kept[:2] == 4).all() and (kept[2] == 8).all()
    d = R.decide(P, kept, np.array([0, 9, 4, 10]), [0.5, 0.9], 15)
    assert (d['order'] == np.arange(10)).all() and (d['set_size'][..., 0] == 5).all() and (d['set_size'][..., 1] == 10).all()
    assert d['rank'][-1].tolist() == [1, 10, 5, 0] and d['totals'][-1, 4] == 1 and d['totals'][-1, 0] == 3
    t = M.classification_calibration(torch.zeros((2, 4, 4, 10)), torch.tensor([0, 9, 4, 10]), [0.5, 0.9], 15)
    assert (t['probs'] == 0.1).all() and t['set_size'].tolist() == [[5, 10]] * 4 and t['rank'].tolist() == [1, 10, 5, 0]


def test_a_row_with_nothing_kept():
    raw = np.random.default_rng(0).standard_normal((2 * 2, 3, 4)).astype(np.float32)
    raw[:2, 1, 0] = np.nan                                             # chain 0 loses row 1
    raw[:, 2, 3] = np.inf                                              # every chain loses row 2
    P, kept = R.probs(raw, 2, 2)
    assert kept.tolist() == [[2, 0, 0], [2, 2, 0], [4, 2, 0]]
    assert np.isnan(P[0, 1]).all() and np.isnan(P[:, 2]).all() and np.isfinite(P[2, 1]).all() and (P[2, 1] == P[1, 1]).all()
    d = R.decide(P, kept, np.array([1, 2, 3]), [0.9], 5)
    assert d['totals'][:, 0].tolist() == [1, 2, 2] and d['rank'][:, 2].tolist() == [0, 0, 0] and (d['set_size'][:, 2] == 0).all()


# ---------------------------------------------------------------- the torch form -----------------
@pytest.mark.parametrize('scale', [1.0, 50.0])
def test_torch_form_matches_the_reference(scale):
    rng = np.random.default_rng(3)
    C_, S_, N, K = 3, 4, 60, 7
    raw = (scale * rng.standard_normal((C_, S_, N, K))).astype(np.float32)
    raw[0, 1, 3, 2] = np.nan
    raw[1, :, 5, :] = np.inf
    raw[:, :, 7, 0] = -np.inf
    y = rng.integers(0, K, N)
    y[[2, 9]] = [-1, K]
    cov = [0.5, 0.75, 0.9]
    P, kept = R.probs(raw.reshape(C_ * S_, N, K), C_, S_)
    t = {k: v.numpy() for k, v in M.classification_calibration(torch.from_numpy(raw), torch.from_numpy(y), cov, 12, budget=1 << 16).items()}
    assert (np.isnan(t['probs']) == np.isnan(P)).all() and np.nanmax(np.abs(t['probs'] - P)) <= 1e-14 and (t['kept'] == kept).all()
    d = R.decide(t['probs'], t['kept'], y, cov, 12)                     # discrete outputs from the same probabilities
    for k in ('order', 'set_size', 'rank'):
        assert t[k].dtype == np.int32 and (t[k] == d[k][-1]).all(), k
    np.testing.assert_allclose(t['totals'], d['totals'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(t['bins'], d['bins'], rtol=1e-12, atol=0)
    assert d['totals'][:, 4].tolist() == [2, 2, 2, 2] and d['totals'][-1, 0] == N - 3


def test_ece_is_zero_on_exactly_calibrated_bins():
    """Two classes, four rows at confidence 0.75 of which three are right, eight at 0.5 of which four are: every bin's
    accuracy is its confidence."""
    P = np.array([[0.75, 0.25]] * 4 + [[0.5, 0.5]] * 8)[None]
    y = np.array([0, 0, 0, 1] + [0, 1] * 4)
    d = R.decide(P, np.ones((1, 12), dtype=np.int32), y, [0.6, 0.9], 4)
    s = M.calibration_summary({'totals': d['totals'], 'bins': d['bins'], 'coverages': [0.6, 0.9]})[0]
    assert s['rows'] == 12 and s['acc'] == 7 / 12 and s['ece'] == 0.0 and s['mce'] == 0.0
    assert d['bins'][0, 3].tolist() == [4.0, 3.0, 3.0] and d['bins'][0, 2].tolist() == [8.0, 4.0, 4.0]
    assert s['coverage_0.6'] == 11 / 12 and s['coverage_0.9'] == 1.0 and s['set_size_0.6'] == (4 * 1 + 8 * 2) / 12 and s['set_size_0.9'] == 2.0
    assert s['cal_error'] == pytest.approx(np.sqrt(((0.6 - 11 / 12) ** 2 + (0.9 - 1.0) ** 2) / 2), abs=1e-15)
    # one wrong row more in the upper bin: its gap is 1 / 4 of four rows
    y[0] = 1
    d = R.decide(P, np.ones((1, 12), dtype=np.int32), y, [0.6, 0.9], 4)
    s = M.calibration_summary({'totals': d['totals'], 'bins': d['bins'], 'coverages': [0.6, 0.9]})[0]
    assert s['ece'] == pytest.approx(1.0 / 12, abs=1e-15) and s['mce'] == pytest.approx(0.25, abs=1e-15)


# ---------------------------------------------------------------- the library's host side -----------------
def test_library_exports_the_three_symbols_under_abi_10():
    from mile_amd import _lib
    from mile_amd._build import build_library
    build_library()
    lib = _lib.load_library()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert _lib.SIGNATURES['mile_calibration'] == (i32, [p, i32, i64, i64, i32, p, p, i32, i32, p, p, p, p, p, p, p, p])
    assert _lib.SIGNATURES['mile_calibration_stream'] == (i32, [p, p, i32, i64, p, p, i64, p, i32, i32, p, p, p, p, p, p, p, i64, i64, p])
    assert _lib.SIGNATURES['mile_calibration_stream_workspace'] == (i64, [p, i32, i64, i64])
    assert lib.mile_abi_version() == _lib.ABI_VERSION == 10         # new symbols under the same ABI
    header = ' '.join((ROOT / 'include' / 'mile_hip.h').read_text().split())
    assert '#define MILE_ABI_VERSION 10' in header
    assert ('int32_t mile_calibration(const float *raw, int32_t C, int64_t S, int64_t N, int32_t K, const void *y, '
            'const double *coverages, int32_t Q, int32_t n_bins,') in header
    assert 'int64_t mile_calibration_stream_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N);' in header
    assert 'mile_loo_stream and mile_calibration_stream share' in header   # the sentence that lists the workspace's users


def _cases(p, lv):
    return [('null coverages', dict(cov=None), 'null argument'), ('no output', dict(outs=(None,) * 7), 'no output asked for'),
            ('C = 0', dict(C_=0), 'C out of range'), ('C = 65536', dict(C_=65536), 'C out of range'),
            ('S = 0', dict(S=0), 'S out of range'), ('N = 0', dict(N=0), 'N out of range'), ('N = 2^30', dict(N=1 << 30), 'N out of range'),
            ('C * S', dict(C_=65535, S=1 << 20), 'C * S'),
            ('Q = 0', dict(Q=0), 'Q out of range'), ('Q = 17', dict(Q=17, cov=lv(*np.linspace(0.1, 0.9, 17))), 'Q out of range'),
            ('not increasing', dict(cov=lv(0.9, 0.5)), 'strictly increasing'), ('equal', dict(cov=lv(0.5, 0.5)), 'strictly increasing'),
            ('level 0', dict(cov=lv(0.0, 0.5)), 'strictly inside'), ('level 1', dict(cov=lv(0.5, 1.0)), 'strictly inside'),
            ('level NaN', dict(cov=lv(float('nan'), 0.5)), 'strictly inside'),
            ('n_bins = 0', dict(n_bins=0), 'n_bins out of range'), ('n_bins = 65', dict(n_bins=65), 'n_bins out of range'),
            ('rank without y', dict(y=None, outs=(p, None, None, None, p, None, None)), 'need y'),
            ('totals without y', dict(y=None, outs=(None,) * 5 + (p, None)), 'need y'),
            ('bins without y', dict(y=None, outs=(None,) * 6 + (p,)), 'need y')]


def test_calibration_refuses_bad_arguments_without_a_gpu():
    from mile_amd import _lib
    lib = _lib.load_library()
    buf = (C.c_double * 1024)()
    p = C.cast(buf, C.c_void_p)
    lv = lambda *v: (C.c_double * len(v))(*v)

    def call(raw=p, C_=2, S=3, N=4, K=3, y=p, cov=lv(0.5, 0.9), Q=2, n_bins=15, outs=(p,) * 7):
        return lib.mile_calibration(raw, C_, S, N, K, y, cov, Q, n_bins, *outs, None)
    cases = _cases(p, lv) + [('null raw', dict(raw=None), 'null argument'), ('K = 1', dict(K=1), 'K out of range'),
                             ('K = 65', dict(K=65), 'K out of range')]
    for tag, kw, text in cases:
        assert call(**kw) == -1, tag
        msg = lib.mile_last_error().decode()
        assert msg.startswith('mile_calibration: ') and text in msg, (tag, msg)


def test_calibration_stream_refuses_bad_arguments_without_a_gpu():
    from mile_amd import _lib
    lib = _lib.load_library()
    buf = (C.c_double * 1024)()
    p = C.cast(buf, C.c_void_p)
    lv = lambda *v: (C.c_double * len(v))(*v)

    def call(hh, theta=p, C_=2, S=3, X=p, y=p, N=4, cov=lv(0.5, 0.9), Q=2, n_bins=15, outs=(p,) * 7, passes=0, tile=0):
        return lib.mile_calibration_stream(hh, theta, C_, S, X, y, N, cov, Q, n_bins, *outs, passes, tile, None)
    h = C.c_void_p()
    assert lib.mile_create(C.byref(_fcn_cspec(5, (16, 16, 3), task=1)), 0, C.byref(h)) == 0
    try:
        cases = [(t, h, kw, m) for t, kw, m in _cases(p, lv)]
        cases += [('null handle', None, {}, 'null argument'), ('null theta', h, dict(theta=None), 'null argument'),
                  ('null X', h, dict(X=None), 'null argument'), ('passes < 0', h, dict(passes=-1), 'max_draws_per_pass < 0'),
                  ('tile < 0', h, dict(tile=-1), 'max_rows_per_tile < 0')]
        for tag, hh, kw, text in cases:
            assert call(hh, **kw) == -1, tag
            msg = lib.mile_last_error().decode()
            assert msg.startswith('mile_calibration_stream: ') and text in msg, (tag, msg)
        # covertype-like: within the budget whatever S is -- 128 MiB of logits, 128 MiB of state, the partial sums
        ws = [lib.mile_calibration_stream_workspace(h, 12, S, 100000) for S in (10, 1000, 100000)]
        assert 0 < ws[0] <= ws[1] == ws[2] <= (320 << 20), ws
        for C_, S, N in ((0, 3, 4), (65536, 3, 4), (2, 0, 4), (2, 3, 0), (2, 3, 1 << 30)):
            assert lib.mile_calibration_stream_workspace(h, C_, S, N) == -1
        assert lib.mile_calibration_stream_workspace(None, 2, 3, 4) == -1
    finally:
        lib.mile_destroy(h)
    # a regression handle, and one whose output width is beyond a wave
    for cs, text in ((_fcn_cspec(5, (16, 16, 2)), 'needs a classification model'), (_fcn_cspec(5, (16, 80), task=1), 'K out of range')):
        assert lib.mile_create(C.byref(cs), 0, C.byref(h)) == 0
        try:
            assert call(h) == -1 and text in lib.mile_last_error().decode()
            assert lib.mile_calibration_stream_workspace(h, 2, 3, 4) == -1
        finally:
            lib.mile_destroy(h)
    # frozen tables not set: a state error, after the argument checks
    assert lib.mile_create(C.byref(_attn_pre_cspec()), 0, C.byref(h)) == 0, lib.mile_last_error()
    try:
        assert call(h, n_bins=0) == -1 and call(h) == -2
    finally:
        lib.mile_destroy(h)


# ---------------------------------------------------------------- the tools -----------------
def test_parsers_accept_calibration_and_sets():
    import evaluate as EV
    import predict as PR
    ap = EV.build_parser()
    assert ap.parse_args(['-e', 'x']).calibration is None           # opt-in
    assert ap.parse_args(['-e', 'x', '--calibration']).calibration == 15
    args = ap.parse_args(['-e', 'x', '--calibration', '10', '--coverages', '0.5', '0.9'])
    assert args.calibration == 10 and args.coverages == [0.5, 0.9] and args.intervals is False
    pp = PR.build_parser()
    assert pp.parse_args(['-e', 'x', '-i', 't.npy']).sets is None
    assert pp.parse_args(['-e', 'x', '-i', 't.npy', '--sets', '0.5', '0.9']).sets == [0.5, 0.9]
    rng = np.random.default_rng(1)
    res = M.classification_calibration(torch.from_numpy(rng.standard_normal((3, 4, 50, 5)).astype(np.float32)),
                                       torch.from_numpy(rng.integers(0, 5, 50)), [0.5, 0.9], 10)
    keys, arrays = EV.calibration_metrics(res, 10)
    assert sorted(arrays) == ['bins', 'coverages', 'kept', 'order', 'probs', 'rank', 'set_size', 'totals']
    assert arrays['probs'].shape == (50, 5) and arrays['probs'].dtype == np.float32 and arrays['bins'].shape == (4, 10, 3)
    ens = M.calibration_summary(res)[-1]
    assert all(keys['calibration_' + k] == v for k, v in ens.items()) and len(keys['calibration_per_chain_ece']) == 3
    assert keys['calibration_per_chain_nll_median'] == float(np.median(keys['calibration_per_chain_nll']))
    assert keys['calibration_coverage_0.9'] >= 0.9 - 3 * np.sqrt(0.09 / 50) and keys['calibration_set_size_0.5'] >= 1.0


@pytest.mark.parametrize('tool,extra,flag', [('evaluate.py', ['--calibration'], '--calibration'),
                                             ('predict.py', ['-i', 'none.npy', '--sets', '0.9'], '--sets')])
def test_tools_refuse_a_regression_experiment(tmp_path, tool, extra, flag):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    assert cfg['data']['task'] == 'regr'
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, str(ROOT / tool), '-e', str(tmp_path)] + extra, capture_output=True, text=True, cwd=ROOT,
                       timeout=120)
    assert r.returncode != 0 and flag in r.stderr and 'classification' in r.stderr, r.stderr[-2000:]
