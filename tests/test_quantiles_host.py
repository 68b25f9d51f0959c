"""The fp64 reference of the ensemble's predictive quantiles and PIT (tests/quantile_ref.py) against closed forms, the torch
restatements of mile_amd.metrics against it, the interval levels, and the host side of mile_mixture_quantiles /
mile_predict_quantiles: exports, bindings and every argument refusal through ctypes on handles created without a GPU."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy.special import ndtri

from mile_amd import metrics as M
from tests import quantile_ref as QR
from tests.test_predict_host import _attn_pre_cspec, _fcn_cspec

ROOT = Path(__file__).resolve().parents[1]
LEVELS = [0.025, 0.05, 0.125, 0.25, 0.5, 0.75, 0.875, 0.95, 0.975]


def _random_raw(S, N, seed):
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal(N)[None] * 2.0 + np.exp(rng.uniform(-2.0, 1.0, N))[None] * rng.standard_normal((S, N))
    return np.stack([mu, rng.uniform(-2.0, 1.0, (S, N))], axis=-1)


# ---------------------------------------------------------------- the reference -----------------
def test_one_component_is_its_normal_quantile():
    raw = _random_raw(1, 11, 0)
    exact = raw[0, :, :1] + ndtri(np.array(LEVELS))[None] * np.exp(raw[0, :, 1:])
    np.testing.assert_allclose(QR.quantiles(raw, LEVELS), exact, rtol=1e-14, atol=0)


def test_identical_components_behave_as_one():
    one = _random_raw(1, 11, 1)
    np.testing.assert_allclose(QR.quantiles(np.repeat(one, 7, axis=0), LEVELS), QR.quantiles(one, LEVELS), rtol=1e-14, atol=0)
    y = np.linspace(-3, 3, 11)
    np.testing.assert_allclose(QR.pit(np.repeat(one, 7, axis=0), y), QR.pit(one, y), rtol=1e-14, atol=0)


def test_symmetric_pair_has_its_median_at_the_midpoint():
    rng = np.random.default_rng(2)
    a, ls = rng.standard_normal(9) * 5, rng.uniform(-1, 1, 9)
    b = a + np.exp(ls) * rng.uniform(0.5, 3.0, 9)                  # (overlapping: far apart, F is flat at 1/2 and the median is not unique)
    raw = np.stack([np.stack([a, ls], axis=-1), np.stack([b, ls], axis=-1)])
    med = QR.quantiles(raw, [0.5])[:, 0]
    np.testing.assert_allclose(med, 0.5 * (a + b), rtol=0, atol=1e-13 * np.abs(a - b).max())
    np.testing.assert_allclose(QR.pit(raw, 0.5 * (a + b)), 0.5, rtol=0, atol=1e-15)


def test_inside_the_interval_exactly_when_the_pit_says_so():
    raw = _random_raw(40, 500, 3)
    rng = np.random.default_rng(4)
    pick = rng.integers(0, 40, 500)
    y = raw[pick, np.arange(500), 0] + np.exp(raw[pick, np.arange(500), 1]) * rng.standard_normal(500)
    pit = QR.pit(raw, y)
    for c in (0.5, 0.75, 0.9, 0.95):
        q = QR.quantiles(raw, M.get_quantiles(c).numpy())
        inside = (q[:, 0] <= y) & (y <= q[:, 1])
        by_pit = np.abs(pit - 0.5) <= c / 2
        assert 0 < inside.sum() < 500 and (inside == by_pit).all(), c
        assert float(M.coverage_from_pit(torch.from_numpy(pit), [c])[0]) == inside.mean()


def test_nonfinite_draws_leave_their_rows_only():
    raw = _random_raw(6, 5, 5)
    raw[1, 0, 0] = np.nan
    raw[2, 0, 1] = -np.inf
    raw[:, 3, 1] = np.inf
    q = QR.quantiles(raw, LEVELS)
    np.testing.assert_allclose(q[0], QR.quantiles(raw[[0, 3, 4, 5], :1], LEVELS)[0], rtol=1e-14)
    assert np.isnan(q[3]).all() and np.isfinite(q[[0, 1, 2, 4]]).all() and np.isnan(QR.pit(raw, np.zeros(5))[3])


# ---------------------------------------------------------------- the torch restatements -----------------
@pytest.mark.parametrize('S,N', [(1, 5), (9, 13), (200, 7)])
def test_restatements_match_the_reference(S, N):
    raw = _random_raw(S, N, 6 + S)
    raw[0, 0, 1] = -20.0                                           # both clips of sigma
    raw[S - 1, 1, 1] = 20.0
    if S > 2:
        raw[1, 2, 0] = np.nan
    got, dropped = M.mixture_quantiles(torch.from_numpy(raw), LEVELS, return_dropped=True)
    ref = QR.quantiles(raw, LEVELS)
    assert got.dtype == torch.float64 and got.shape == (N, len(LEVELS)) and dropped.dtype == torch.int32
    assert dropped.tolist() == [0, 0, 1 if S > 2 else 0] + [0] * (N - 3)
    np.testing.assert_allclose(got.numpy(), ref, rtol=1e-10, atol=0)
    y = np.linspace(-4, 4, N)
    np.testing.assert_allclose(M.mixture_pit(torch.from_numpy(raw), torch.from_numpy(y)).numpy(), QR.pit(raw, y), rtol=1e-10, atol=0)
    # float32 outputs are read as they are, and the leading axes are draw axes
    r32 = raw.astype(np.float32)
    np.testing.assert_allclose(M.mixture_quantiles(torch.from_numpy(r32), LEVELS).numpy(), QR.quantiles(r32, LEVELS), rtol=1e-10, atol=0)
    if S == 200:
        assert torch.equal(M.mixture_quantiles(torch.from_numpy(raw.reshape(4, 50, N, 2)), LEVELS), got)


def test_restatement_rows_without_a_draw_and_bad_levels():
    raw = _random_raw(4, 3, 9)
    raw[:, 1, 0] = np.inf
    q, dropped = M.mixture_quantiles(torch.from_numpy(raw), [0.1, 0.9], return_dropped=True)
    assert torch.isnan(q[1]).all() and torch.isfinite(q[[0, 2]]).all() and dropped.tolist() == [0, 4, 0]
    assert torch.isnan(M.mixture_pit(torch.from_numpy(raw), torch.zeros(3))[1])
    assert float(M.coverage_from_pit(torch.tensor([0.5, float('nan'), 0.99]), [0.9])[0]) == 0.5      # finite rows only
    for bad in ([0.0, 0.5], [0.5, 1.0], []):
        with pytest.raises(ValueError):
            M.mixture_quantiles(torch.from_numpy(raw), bad)


def test_interval_levels():
    lv = M.interval_levels([0.5, 0.75, 0.9, 0.95])
    assert lv.dtype == torch.float64
    np.testing.assert_allclose(lv.numpy(), [0.025, 0.05, 0.125, 0.25, 0.75, 0.875, 0.95, 0.975], rtol=0, atol=1e-15)
    for c in (0.5, 0.75, 0.9, 0.95):                               # each interval's own two levels are among them, bit for bit
        assert all(float(v) in lv.tolist() for v in M.get_quantiles(c))
    assert M.interval_levels([0.9, 0.9]).tolist() == M.get_quantiles(0.9).tolist()


def test_interval_metrics_keys():
    import evaluate as EV
    assert EV.build_parser().parse_args(['-e', 'x']).intervals is False       # opt-in
    raw = _random_raw(30, 50, 10)
    y = raw[0, :, 0]
    cov = [0.5, 0.9]
    lv = M.interval_levels(cov)
    q, dropped = M.mixture_quantiles(torch.from_numpy(raw), lv, return_dropped=True)
    keys, arrays = EV.interval_metrics(q, M.mixture_pit(torch.from_numpy(raw), torch.from_numpy(y)), dropped, lv, cov)
    assert sorted(keys) == ['intervals_cal_error', 'intervals_coverage_0.5', 'intervals_coverage_0.9', 'intervals_dropped',
                            'intervals_width_0.5', 'intervals_width_0.9']
    assert sorted(arrays) == ['dropped', 'levels', 'pit', 'quantiles'] and arrays['quantiles'].shape == (50, 4)
    inside = (q[:, 0].numpy() <= y) & (y <= q[:, 3].numpy())
    assert keys['intervals_coverage_0.9'] == inside.mean() and 0 < keys['intervals_width_0.5'] < keys['intervals_width_0.9']
    assert keys['intervals_width_0.9'] == pytest.approx(float((q[:, 3] - q[:, 0]).mean()), rel=1e-6)


# ---------------------------------------------------------------- C ABI -----------------
NEW = ('mile_mixture_quantiles', 'mile_predict_quantiles', 'mile_predict_quantiles_workspace')


def test_library_exports_the_three_symbols_under_abi_10():
    from mile_amd import _lib
    from mile_amd._build import build_library
    build_library()
    lib = _lib.load_library()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES['mile_mixture_quantiles'][1]) == 10 and len(_lib.SIGNATURES['mile_predict_quantiles'][1]) == 14
    assert _lib.SIGNATURES['mile_predict_quantiles_workspace'][0] is C.c_int64
    assert lib.mile_abi_version() == _lib.ABI_VERSION == 10         # new symbols under the same ABI
    header = (ROOT / 'include' / 'mile_hip.h').read_text()
    assert '#define MILE_ABI_VERSION 10' in header and all(f'{n}(' in header for n in NEW)


def _levels(*v):
    return (C.c_double * len(v))(*v)


BAD_LEVELS = [('Q = 0', _levels(0.5), 0), ('Q = 33', _levels(*np.linspace(0.01, 0.99, 33)), 33), ('null levels', None, 1),
              ('level 0', _levels(0.0, 0.5), 2), ('level 1', _levels(0.5, 1.0), 2), ('NaN level', _levels(float('nan')), 1),
              ('decreasing', _levels(0.5, 0.25), 2), ('repeated', _levels(0.5, 0.5), 2)]


def test_mixture_quantiles_refuses_bad_arguments_without_a_gpu():
    from mile_amd import _lib
    lib = _lib.load_library()
    buf = (C.c_float * 1024)()
    p = C.cast(buf, C.c_void_p)
    ok = _levels(0.25, 0.75)
    call = lambda raw, S, N, lv, Q, y, quant, pit: lib.mile_mixture_quantiles(raw, S, N, lv, Q, y, quant, pit, None, None)
    cases = [('null raw', (None, 4, 4, ok, 2, p, p, p)), ('S = 0', (p, 0, 4, ok, 2, p, p, p)), ('S < 0', (p, -1, 4, ok, 2, p, p, p)),
             ('S = 2^31', (p, 1 << 31, 4, ok, 2, p, p, p)), ('N = 0', (p, 4, 0, ok, 2, p, p, p)),
             ('N = 2^30', (p, 4, 1 << 30, ok, 2, p, p, p)), ('pit without y', (p, 4, 4, ok, 2, None, p, p)),
             ('no output', (p, 4, 4, ok, 2, p, None, None))]
    cases += [(tag, (p, 4, 4, lv, Q, p, p, p)) for tag, lv, Q in BAD_LEVELS]
    for tag, args in cases:
        assert call(*args) == -1, tag
        assert b'mile_mixture_quantiles' in lib.mile_last_error(), tag


def test_predict_quantiles_refuses_bad_arguments_without_a_gpu():
    from mile_amd import _lib
    lib = _lib.load_library()
    h = C.c_void_p()
    assert lib.mile_create(C.byref(_fcn_cspec(5, (16, 16, 2))), 0, C.byref(h)) == 0
    try:
        buf = (C.c_float * 1024)()
        p = C.cast(buf, C.c_void_p)
        ok = _levels(0.25, 0.75)

        def call(hh, theta, S, X, N, lv, Q, y, quant, pit, passes=0, tile=0):
            return lib.mile_predict_quantiles(hh, theta, S, X, N, lv, Q, y, quant, pit, None, passes, tile, None)
        cases = [('null handle', (None, p, 4, p, 4, ok, 2, p, p, p)), ('null theta', (h, None, 4, p, 4, ok, 2, p, p, p)),
                 ('null X', (h, p, 4, None, 4, ok, 2, p, p, p)), ('S = 0', (h, p, 0, p, 4, ok, 2, p, p, p)),
                 ('S = 2^31', (h, p, 1 << 31, p, 4, ok, 2, p, p, p)), ('N = 0', (h, p, 4, p, 0, ok, 2, p, p, p)),
                 ('N = 2^30', (h, p, 4, p, 1 << 30, ok, 2, p, p, p)), ('pit without y', (h, p, 4, p, 4, ok, 2, None, p, p)),
                 ('no output', (h, p, 4, p, 4, ok, 2, p, None, None)), ('passes < 0', (h, p, 4, p, 4, ok, 2, p, p, p, -1, 0)),
                 ('tile < 0', (h, p, 4, p, 4, ok, 2, p, p, p, 0, -1))]
        cases += [(tag, (h, p, 4, p, 4, lv, Q, p, p, p)) for tag, lv, Q in BAD_LEVELS]
        for tag, args in cases:
            assert call(*args) == -1, tag
            assert b'mile_predict_quantiles' in lib.mile_last_error(), tag
        assert lib.mile_predict_quantiles_workspace(h, 12000, 301) >= 2 * 12000 * 301 * 8
        assert lib.mile_predict_quantiles_workspace(h, 1 << 24, 1000) < (300 << 20)        # tiles: within the budget
        for S, N in ((0, 4), (4, 0), (1 << 31, 4), (4, 1 << 30)):
            assert lib.mile_predict_quantiles_workspace(h, S, N) == -1
        assert lib.mile_predict_quantiles_workspace(None, 4, 4) == -1
    finally:
        lib.mile_destroy(h)
    # a classification handle, and frozen tables not set (argument checks come first)
    assert lib.mile_create(C.byref(_fcn_cspec(5, (16, 3), task=1)), 0, C.byref(h)) == 0
    try:
        assert call(h, p, 4, p, 4, ok, 2, p, p, p) == -1 and b'regression' in lib.mile_last_error()
    finally:
        lib.mile_destroy(h)
    assert lib.mile_create(C.byref(_attn_pre_cspec()), 0, C.byref(h)) == 0, lib.mile_last_error()
    try:
        assert call(h, p, 4, p, 4, ok, 2, p, p, p) == -1          # a classifier: refused as such before its tables are asked for
        assert call(h, None, 4, p, 4, ok, 2, p, p, p) == -1
    finally:
        lib.mile_destroy(h)


# ---------------------------------------------------------------- the tools -----------------
@pytest.mark.parametrize('tool,extra', [('evaluate.py', ['--intervals']), ('predict.py', ['-i', 'none.npy', '--intervals', '0.9'])])
def test_tools_refuse_a_classification_experiment(tmp_path, tool, extra):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'mclmc_covertype_b4.yaml').read_text())
    assert cfg['data']['task'] != 'regr'
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, str(ROOT / tool), '-e', str(tmp_path)] + extra, capture_output=True, text=True, cwd=ROOT,
                       timeout=120)
    assert r.returncode != 0 and '--intervals' in r.stderr and 'regression' in r.stderr, r.stderr[-2000:]
