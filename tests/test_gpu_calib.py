"""mile_calibration / mile_calibration_stream (Engine.calibration, Engine.calibration_stream) against the fp64 restatement of
tests/calib_ref.py (-m gpu): the kernels on given logits in every regime, the non-finite rule, the streamed call bit for bit
under every pass and tile size, end to end through the forward kernels, the shared workspace, the refusals and the two CLIs.

Bounds.  On given fp32 logits ``probs`` is within 1e-12 absolute of the restatement: a per-draw p carries at most ~(K + 4)
ulp of fp64 and a mean no more than its terms, <= 1e-14.  Every discrete output (order, set_size, rank, kept, bin counts, rows
correct, rows covered) equals ``calib_ref.decide`` of the DEVICE's probabilities exactly -- replaying from the device's own
probabilities is what removes the near-boundary flips, so no row is left out -- and the fp64 sums (Brier, NLL, confidence,
set size) are within 1e-12 relative of the same replay.  End to end ``probs`` gets test_gpu_moments.py's bound,
max|out - ref| < 1e-4 max(1, max|ref|), and the mean Brier score and NLL that file's policy: 4x the measured error of the
float32 restatement (the torch form on the float32 oracle forward), which must itself stay below 1e-3 of the value -- both
errors taken per case, the largest over the groups (a single group's float32 error is a mean of signed row errors and can
cancel to a fraction of its neighbours').

Measured on an MI355X: see DESIGN.md section 3.2q."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import attn_ref as RA
from tests import calib_ref as R
from tests.test_gpu_predict import DEV, ROOT, _fcn_engine, _reload, _run

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

COV = (0.5, 0.9, 0.95)
NB = 15
DISCRETE = ('order', 'set_size', 'rank', 'kept')
ALL = ('probs',) + DISCRETE + ('totals', 'bins')
_ENGINE = {}


def _engine():
    """Any engine: calibration needs no handle, only the library and the device."""
    if 'e' not in _ENGINE:
        ospec = O.ModelSpec(5, (16, 16, 2), activation='relu', task='regr')
        _ENGINE['e'] = _fcn_engine(ospec, O.synthetic_problem(ospec, 64, 1, seed=3, theta_scale=0.3), 'mfma_narrow_f32')
    return _ENGINE['e']


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same_bits(tag, a, b):
    for k in ALL:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (tag, k, a[k], b[k])


def _check_replay(tag, got, y, Q, n_bins=NB, cov=COV):
    """Everything behind ``probs`` against calib_ref.decide of the device's own probs: discrete exact, sums at 1e-12 relative."""
    d = R.decide(got['probs'], got['kept'], y, cov, n_bins)
    for k in ('order', 'set_size', 'rank'):
        assert got[k].dtype == np.int32 and (got[k] == d[k][-1]).all(), (tag, k, np.argwhere(got[k] != d[k][-1])[:5])
    t, b = got['totals'], got['bins']
    assert t.shape == d['totals'].shape and b.shape == d['bins'].shape and t.dtype == b.dtype == np.float64
    exact = [0, 1, 4] + list(range(5, 5 + Q))
    assert (t[:, exact] == d['totals'][:, exact]).all(), (tag, 'counts', t[:, exact], d['totals'][:, exact])
    assert (b[..., 0] == d['bins'][..., 0]).all() and (b[..., 2] == d['bins'][..., 2]).all(), (tag, 'bin counts')
    sums = [2, 3] + list(range(5 + Q, 5 + 2 * Q))
    worst = 0.0
    for g_, r_ in ((t[:, sums], d['totals'][:, sums]), (b[..., 1], d['bins'][..., 1])):
        assert (np.isfinite(g_) == np.isfinite(r_)).all() and (g_[~np.isfinite(r_)] == r_[~np.isfinite(r_)]).all(), (tag, g_, r_)
        fin = np.isfinite(r_) & (r_ != 0)
        assert (g_[np.isfinite(r_) & (r_ == 0)] == 0).all()
        if fin.any():
            worst = max(worst, float((np.abs(g_[fin] - r_[fin]) / np.abs(r_[fin])).max()))
    print(f'{tag}: sums against the replay, worst relative error {worst:.2e}')
    assert worst <= 1e-12, (tag, worst)
    return d


# ---- 1. the kernels on given logits -----------------------------------------------------------------------------------------
def _logits(regime, K, N, C_, S_, rng):
    z = rng.standard_normal((C_ * S_, N, K))
    if regime == 'x50':
        z *= 50.0                                                      # saturated: the tail's probabilities are ~1e-100
    elif regime == 'x400':
        z *= 400.0                                                     # exp underflows: exact zeros tie in the tail
    elif regime == 'zero':
        z[:] = 0.0
    elif regime == 'duplicated':
        z[..., 1] = z[..., 0]
        z[..., K - 1] = z[..., 0]
    return np.ascontiguousarray(z.astype(np.float32))


@pytest.mark.parametrize('regime', ['unit', 'x50', 'x400', 'zero', 'duplicated'])
@pytest.mark.parametrize('K,N,C_,S_', [(2, 1, 1, 1), (3, 33, 2, 1), (7, 257, 3, 5), (10, 130, 2, 4), (64, 65, 1, 3)])
def test_given_logits(K, N, C_, S_, regime):
    rng = np.random.default_rng(1000 * K + N)
    raw = _logits(regime, K, N, C_, S_, rng)
    y = rng.integers(0, K, N).astype(np.int32)
    got = _np(_engine().calibration(torch.from_numpy(raw.reshape(C_, S_, N, K)), torch.from_numpy(y), COV, NB))
    P, kept = R.probs(raw, C_, S_)
    assert got['probs'].shape == (C_ + 1, N, K) and got['probs'].dtype == np.float64
    err = float(np.abs(got['probs'] - P).max())
    tag = f'K={K} N={N} C={C_} S={S_} {regime}'
    print(f'{tag}: max|probs - ref| = {err:.2e}')
    assert err <= 1e-12, (tag, err)
    assert got['kept'].dtype == np.int32 and (got['kept'] == kept).all() and (kept[:C_] == S_).all()
    d = _check_replay(tag, got, y, len(COV))
    assert (got['totals'][:, 0] == N).all() and (got['totals'][:, 4] == 0).all()       # no row is left out anywhere
    if regime == 'zero':                                                # every class of a row goes through the same arithmetic
        assert (got['order'] == np.arange(K)).all() and np.abs(got['probs'] - 1.0 / K).max() <= 1e-15
        if (C_, S_) in ((1, 1), (2, 1), (2, 4)):                        # every sum of 1 / K on the way is exact, or rounds back
            assert (got['probs'] == 1.0 / K).all()
        if K == 10:                                                     # nine fp64 additions of 0.1 stay below 0.9
            assert (got['set_size'] == [5, 10, 10]).all()
    if regime == 'duplicated' and K > 2:                                # equal probabilities: the lower index first
        o = got['order']
        pos = lambda k: np.argmax(o == k, axis=1)
        assert (got['probs'][..., 0] == got['probs'][..., 1]).all() and (pos(0) + 1 == pos(1)).all() and (pos(1) + 1 == pos(K - 1)).all()
    if regime == 'x400' and K > 2 and S_ <= 3:                          # the inputs are what they are called
        assert (got['probs'] == 0.0).any() and (got['set_size'] < K).all()


def test_without_labels_and_other_levels():
    rng = np.random.default_rng(5)
    raw = _logits('unit', 7, 70, 2, 3, rng)
    eng = _engine()
    a = _np(eng.calibration(torch.from_numpy(raw.reshape(2, 3, 70, 7)), None, [0.3], 1))
    assert sorted(a) == ['coverages', 'kept', 'order', 'probs', 'set_size'] and a['set_size'].shape == (70, 1)
    d = R.decide(a['probs'], a['kept'], None, [0.3], 1)
    assert (a['order'] == d['order'][-1]).all() and (a['set_size'] == d['set_size'][-1]).all()
    y = rng.integers(-1, 8, 70).astype(np.int32)                        # some labels outside [0, K)
    cov = tuple(np.linspace(0.05, 0.999, 16))
    b = _np(eng.calibration(torch.from_numpy(raw.reshape(2, 3, 70, 7)), torch.from_numpy(y), cov, 64))
    _check_replay('16 levels, 64 bins, bad labels', b, y, 16, 64, cov)
    bad = int(((y < 0) | (y >= 7)).sum())
    assert bad > 0 and (b['totals'][:, 4] == bad).all() and (b['totals'][:, 0] == 70 - bad).all() and (b['rank'][(y < 0) | (y >= 7)] == 0).all()


# ---- 2. non-finite draws ----------------------------------------------------------------------------------------------------
def test_nonfinite_draws_are_left_out_per_draw_and_row():
    C_, S_, N, K = 3, 4, 9, 4
    rng = np.random.default_rng(11)
    raw = _logits('unit', K, N, C_, S_, rng).reshape(C_, S_, N, K)
    raw[0, 0, 1, 2] = np.nan                                           # (chain 0, row 1) loses two draws
    raw[0, 2, 1, 0] = np.inf
    raw[1, :, 2, 3] = -np.inf                                          # (chain 1, row 2) loses all: the ensemble skips the chain there
    raw[:, :, 5, 1] = np.nan                                           # row 5 loses every draw of every chain
    y = rng.integers(0, K, N).astype(np.int32)
    got = _np(_engine().calibration(torch.from_numpy(raw), torch.from_numpy(y), COV, NB))
    P, kept = R.probs(raw.reshape(C_ * S_, N, K), C_, S_)
    want = np.full((C_ + 1, N), S_, dtype=np.int32)
    want[C_] = C_ * S_
    want[0, 1], want[C_, 1] = 2, C_ * S_ - 2
    want[1, 2], want[C_, 2] = 0, (C_ - 1) * S_
    want[:, 5] = 0
    assert (kept == want).all() and (got['kept'] == want).all(), got['kept']
    assert (np.isnan(got['probs']) == np.isnan(P)).all() and np.isnan(got['probs'][1, 2]).all() and np.isnan(got['probs'][:, 5]).all()
    assert np.isfinite(got['probs'][C_, 2]).all()
    assert float(np.nanmax(np.abs(got['probs'] - P))) <= 1e-12
    _check_replay('non-finite', got, y, len(COV))
    assert got['totals'][:, 0].tolist() == [N - 1, N - 2, N - 1, N - 1]
    assert got['rank'][5] == 0 and (got['set_size'][5] == 0).all() and (got['order'][5] == np.arange(K)).all()


def test_logits_beyond_the_budget_are_walked_in_tiles_of_their_own_rows():
    """C = 1024 members, K = 64: a row's sums, counts and records take 577 584 bytes, so the 128 MiB of a tile hold 232 rows,
    192 in whole workgroups of 64.  N = 193 is that tile and one row more: mile_calibration walks the caller's logits
    (ld = N) in two tiles.  A row's outputs depend on its own logits only, so they are, bit for bit, those of the call on each
    tile's rows alone; the counts among totals and bins are exact sums of 0 / 1 and add up over the tiles."""
    C_, S_, K, Q = 1024, 1, 64, len(COV)
    tile = (128 << 20) // (C_ * (K * 8 + 4) + (C_ + 1) * 48) // 64 * 64
    N = tile + 1
    assert tile == 192
    gen = torch.Generator(device=DEV).manual_seed(13)
    raw = torch.randn(C_, S_, N, K, device=DEV, generator=gen)
    y = torch.randint(0, K, (N,), device=DEV, generator=gen, dtype=torch.int32)
    eng = _engine()
    whole = _np(eng.calibration(raw, y, COV, NB))
    parts = [_np(eng.calibration(raw[:, :, r0:r0 + tile].contiguous(), y[r0:r0 + tile], COV, NB)) for r0 in range(0, N, tile)]
    assert (whole['kept'] == S_ * np.array([1] * C_ + [C_])[:, None]).all() and np.isfinite(whole['probs']).all()
    for k, axis in (('probs', 1), ('kept', 1), ('order', 0), ('set_size', 0), ('rank', 0)):
        both = np.concatenate([p[k] for p in parts], axis=axis)
        assert whole[k].dtype == both.dtype and whole[k].tobytes() == both.tobytes(), k
    counts = [0, 1, 4] + list(range(5, 5 + 2 * Q))                         # rows counted, correct, bad labels, covered, set sizes
    assert (whole['totals'][:, counts] == sum(p['totals'][:, counts] for p in parts)).all()
    assert (whole['bins'][:, :, [0, 2]] == sum(p['bins'][:, :, [0, 2]] for p in parts)).all()
    assert whole['totals'][:, 0].tolist() == [N] * (C_ + 1)


# ---- 3. the streamed call ---------------------------------------------------------------------------------------------------
C_ST, S_ST, N_ST = 2, 3, 130
FCN = {'tanh-3': (7, (40, 40, 3), 'tanh'), 'sigmoid-7': (11, (32, 7), 'sigmoid')}


@functools.lru_cache(maxsize=None)
def _fcn_case(name):
    F, hs, act = FCN[name]
    ospec = O.ModelSpec(F, hs, activation=act, task='classification')
    prob = O.synthetic_problem(ospec, 64, C_ST * S_ST, seed=3, theta_scale=0.3)
    test = O.synthetic_problem(ospec, N_ST, 1, seed=4)
    return ospec, prob, np.ascontiguousarray(test['X']), np.ascontiguousarray(test['y']).astype(np.int32)


def _attn_case():
    from mile_amd.engine import Engine
    from mile_amd.spec import AttentionSpec
    spec = AttentionSpec(100, 30, 16, 4, 16, n_classes=3, projection_dim=(8,), use_bias=True, prior='Normal', prior_scale=0.2)
    prob = RA.synthetic_problem(spec, 20, C_ST * S_ST, seed=6)
    test = RA.synthetic_problem(spec, N_ST, 1, seed=7)
    eng = Engine(spec, torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV)
    assert eng.grad_kernel == 'attn_f32'
    return eng, prob['theta0'], test['X'], np.ascontiguousarray(test['y']).astype(np.int32)


@pytest.mark.parametrize('name', list(FCN) + ['attn'])
def test_stream_is_calibration_of_the_predicted_logits_for_every_pass_and_tile(name):
    if name == 'attn':
        eng, theta, X, y = _attn_case()
    else:
        ospec, prob, X, y = _fcn_case(name)
        eng, theta = _fcn_engine(ospec, prob, 'mfma_narrow_f32'), prob['theta0']
    th = torch.from_numpy(theta).reshape(C_ST, S_ST, -1)
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    raw = eng.predict(th, Xt)
    assert raw.shape[:3] == (C_ST, S_ST, N_ST)
    alone = _np(eng.calibration(raw, yt, COV, NB))
    assert np.isfinite(alone['probs']).all() and (alone['kept'][:C_ST] == S_ST).all() and (alone['totals'][:, 0] == N_ST).all()
    for draws in (0, 1, 2):
        for rows in (0, 32, 33):                                       # at N = 130: four tiles of 32 and one of 2; three of 33 and one of 31
            got = _np(eng.calibration_stream(th, Xt, yt, COV, NB, max_draws_per_pass=draws, max_rows_per_tile=rows))
            _same_bits(f'{name}: passes of {draws}, tiles of {rows}', got, alone)
    assert eng.calibration_stream_workspace(C_ST, S_ST, N_ST) > 0


# ---- 4. end to end against the fp64 forward ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(FCN))
def test_stream_end_to_end_against_the_fp64_forward(name):
    from mile_amd import metrics as M
    ospec, prob, X, y = _fcn_case(name)
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    K = ospec.hidden_structure[-1]
    out64 = O.mlp_forward(ospec, prob['theta0'].astype(np.float64), X.astype(np.float64))          # [C * S, N, K]
    out32 = O.mlp_forward(ospec, prob['theta0'], X)
    P, kept = R.probs(out64, C_ST, S_ST)
    ref = R.decide(P, kept, y, COV, NB)['totals']
    rest = M.classification_calibration(torch.from_numpy(np.ascontiguousarray(out32, dtype=np.float32)).reshape(C_ST, S_ST, N_ST, K),
                                        torch.from_numpy(y), COV, NB)['totals'].numpy()
    got = _np(eng.calibration_stream(torch.from_numpy(prob['theta0']).reshape(C_ST, S_ST, -1), torch.from_numpy(X), torch.from_numpy(y), COV, NB))
    err, bound = float(np.abs(got['probs'] - P).max()), 1e-4 * max(1.0, float(np.abs(P).max()))
    print(f'{name} probs: max|out - ref| = {err:.3e}, bound {bound:.3e}')
    assert err < bound, (name, err, bound)
    assert (got['totals'][:, 0] == N_ST).all() and (ref[:, 0] == N_ST).all()
    for col, what in ((2, 'brier'), (3, 'nll')):                       # per case: the largest error over the groups, on both sides
        v = ref[:, col] / N_ST
        e32 = float(np.abs(rest[:, col] - ref[:, col]).max()) / N_ST
        e = float(np.abs(got['totals'][:, col] - ref[:, col]).max()) / N_ST
        print(f'{name} mean {what}: ref per group {v}, device error {e:.3e}, float32 restatement {e32:.3e}, bound {4.0 * e32:.3e}')
        assert e32 <= 1e-3 * np.abs(v).min(), (name, what, 'badly chosen inputs', e32, v)
        assert e <= 4.0 * e32, (name, what, e, 4.0 * e32)


# ---- 5. one workspace for every streamed call -------------------------------------------------------------------------------
def test_streamed_calls_share_one_workspace():
    ospec, prob, X, y = _fcn_case('tanh-3')
    th3 = torch.from_numpy(prob['theta0']).reshape(C_ST, S_ST, -1)
    th, Xt, yt = torch.from_numpy(prob['theta0']), torch.from_numpy(X), torch.from_numpy(y)
    calls = {'moments': lambda e: {'m': e.predict_moments(th, Xt).cpu().numpy()},
             'calibration': lambda e: {k: v for k, v in _np(e.calibration_stream(th3, Xt, yt, COV, NB)).items()},
             'loo': lambda e: _np(e.loo_stream(th, Xt, yt))}
    fresh = {k: fn(_fcn_engine(ospec, prob, 'mfma_narrow_f32')) for k, fn in calls.items()}
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    for k in ('moments', 'calibration', 'loo', 'calibration', 'moments', 'loo', 'calibration'):
        got = calls[k](eng)
        for name, v in got.items():
            assert v.tobytes() == fresh[k][name].tobytes(), (k, name)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from mile_amd import _lib
    ospec, prob, X, y = _fcn_case('tanh-3')
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    K = 3
    th = torch.from_numpy(prob['theta0']).to(DEV)
    Xt, yt = torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)
    raw = eng.predict(th.reshape(C_ST, S_ST, -1), Xt).contiguous()
    p = lambda t: C.c_void_p(t.data_ptr())
    lv = lambda *v: (C.c_double * len(v))(*v)
    probs = torch.empty((C_ST + 1, N_ST, K), dtype=torch.float64, device=DEV)
    totals = torch.empty((C_ST + 1, 5 + 2 * 16), dtype=torch.float64, device=DEV)
    ok = dict(raw=p(raw), C=C_ST, S=S_ST, N=N_ST, K=K, y=p(yt), cov=lv(0.5, 0.9), Q=2, n_bins=15, probs=p(probs), totals=None)

    def given(**kw):
        a = dict(ok, **kw)
        return eng.lib.mile_calibration(a['raw'], a['C'], a['S'], a['N'], a['K'], a['y'], a['cov'], a['Q'], a['n_bins'], a['probs'],
                                        None, None, None, None, a['totals'], None, None)

    def stream(**kw):
        a = dict(ok, theta=p(th), X=p(Xt), draws=0, rows=0)
        a.update(kw)
        return eng.lib.mile_calibration_stream(eng._h, a['theta'], a['C'], a['S'], a['X'], a['y'], a['N'], a['cov'], a['Q'], a['n_bins'],
                                               a['probs'], None, None, None, None, a['totals'], None, a['draws'], a['rows'], None)

    cases = [('null', dict(raw=None, theta=None), 'null argument'), ('null coverages', dict(cov=None), 'null argument'),
             ('no output', dict(probs=None), 'no output asked for'),
             ('C = 0', dict(C=0), 'C out of range'), ('C = 65536', dict(C=65536), 'C out of range'),
             ('S = 0', dict(S=0), 'S out of range'), ('N = 0', dict(N=0), 'N out of range'), ('N = 2^30', dict(N=1 << 30), 'N out of range'),
             ('Q = 0', dict(Q=0), 'Q out of range'), ('Q = 17', dict(Q=17, cov=lv(*np.linspace(0.1, 0.9, 17))), 'Q out of range'),
             ('not increasing', dict(cov=lv(0.9, 0.5)), 'strictly increasing'), ('equal', dict(cov=lv(0.5, 0.5)), 'strictly increasing'),
             ('level 0', dict(cov=lv(0.0, 0.5)), 'strictly inside'), ('level 1', dict(cov=lv(0.5, 1.0)), 'strictly inside'),
             ('level NaN', dict(cov=lv(0.5, float('nan'))), 'strictly inside'),
             ('n_bins = 0', dict(n_bins=0), 'n_bins out of range'), ('n_bins = 65', dict(n_bins=65), 'n_bins out of range'),
             ('totals without y', dict(y=None, totals=p(totals)), 'need y')]
    for tag, kw, msg in cases:
        for name, fn in (('mile_calibration', given), ('mile_calibration_stream', stream)):
            rc = fn(**{k: v for k, v in kw.items() if k != ('theta' if fn is given else 'raw')})
            text = eng.lib.mile_last_error().decode()
            print(tag, name, rc, text)
            assert rc == -1 and text.startswith(name + ': ') and msg in text, (tag, name, rc, text)
    for tag, kw, msg in [('K = 1', dict(K=1), 'K out of range'), ('K = 65', dict(K=65), 'K out of range')]:
        assert given(**kw) == -1 and msg in eng.lib.mile_last_error().decode(), tag
    for tag, kw, msg in [('draws < 0', dict(draws=-1), 'max_draws_per_pass < 0'), ('rows < 0', dict(rows=-1), 'max_rows_per_tile < 0')]:
        assert stream(**kw) == -1 and msg in eng.lib.mile_last_error().decode(), tag
    assert eng.calibration_stream_workspace(0, S_ST, N_ST) == -1
    # a regression handle is refused, by the library
    rspec = O.ModelSpec(5, (16, 16, 2), activation='relu', task='regr')
    rprob = O.synthetic_problem(rspec, 64, 2, seed=3, theta_scale=0.3)
    reng = _fcn_engine(rspec, rprob, 'mfma_narrow_f32')
    with pytest.raises(_lib.MileHipError, match='libmile_hip error -1: mile_calibration_stream: needs a classification model'):
        reng.calibration_stream(torch.from_numpy(rprob['theta0']).reshape(1, 2, -1), torch.from_numpy(rprob['X']))
    assert reng.calibration_stream_workspace(1, 2, 64) == -1
    with pytest.raises(ValueError):
        eng.calibration(raw, yt, np.linspace(0.1, 0.9, 17))
    # the handle then runs a valid call, and one output alone is a call like any other
    assert stream() == 0
    full = eng.calibration_stream(th.reshape(C_ST, S_ST, -1), Xt, yt, (0.5, 0.9))
    torch.cuda.synchronize()
    assert probs.cpu().numpy().tobytes() == full['probs'].cpu().numpy().tobytes()
    assert full['probs'].cpu().numpy().tobytes() == eng.calibration(raw, yt, (0.5, 0.9))['probs'].cpu().numpy().tobytes()


# ---- 7. the CLIs ------------------------------------------------------------------------------------------------------------
def test_evaluate_and_predict_clis(tmp_path):
    import yaml
    from mile_amd import metrics as M
    rng = np.random.default_rng(0)
    N, F, K = 400, 5, 3
    X = rng.standard_normal((N, F))
    labels = np.argmax(1.5 * X @ rng.standard_normal((F, K)) + rng.gumbel(size=(N, K)), axis=1)
    np.save(tmp_path / 'three.npy', np.concatenate([X, labels[:, None]], axis=1).astype(np.float32))
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['experiment_name'] = 'three_classes'
    cfg['data'].update(path=str(tmp_path / 'three.npy'), source='local', task='class')
    cfg['model']['hidden_structure'] = [16, 16, K]
    cfg['training']['sampler'].update(warmup_steps=40, n_samples=60, n_chains=2)           # thinning 10: 6 draws kept per chain
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    _run([ROOT / 'train.py', '-c', tmp_path / 'cfg.yaml', '-d', '1'])
    exp = tmp_path / 'three_classes'
    _run([ROOT / 'evaluate.py', '-e', exp])
    plain = json.loads((exp / 'metrics.json').read_text())
    assert not (exp / 'calibration.npz').exists() and not any(k.startswith('calibration_') for k in plain)
    _run([ROOT / 'evaluate.py', '-e', exp, '--calibration', '--coverages', '0.5', '0.9'])
    m = json.loads((exp / 'metrics.json').read_text())
    assert {k: v for k, v in m.items() if not k.startswith('calibration_')} == plain
    eng, samples, x, y = _reload(exp, 'test')
    Nt, C_ = x.shape[0], samples.shape[0]
    z = np.load(exp / 'calibration.npz')
    assert sorted(z.files) == ['bins', 'coverages', 'kept', 'order', 'probs', 'rank', 'set_size', 'totals']
    assert z['probs'].shape == (Nt, K) and z['probs'].dtype == np.float32 and z['order'].shape == (Nt, K) and z['set_size'].shape == (Nt, 2)
    assert z['rank'].shape == (Nt,) and z['kept'].shape == (C_ + 1, Nt) and z['bins'].shape == (C_ + 1, 15, 3) and z['totals'].shape == (C_ + 1, 9)
    assert z['coverages'].tolist() == [0.5, 0.9] and C_ == 2
    ref = _np(M.classification_calibration(eng.predict(torch.from_numpy(samples), torch.from_numpy(x)), torch.from_numpy(y), [0.5, 0.9], 15))
    for k in DISCRETE:
        assert (z[k] == ref[k]).all(), k
    assert (z['totals'][:, [0, 1, 4, 5, 6]] == ref['totals'][:, [0, 1, 4, 5, 6]]).all() and (z['bins'][..., [0, 2]] == ref['bins'][..., [0, 2]]).all()
    np.testing.assert_allclose(z['totals'], ref['totals'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(z['bins'], ref['bins'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(z['probs'], ref['probs'][-1].astype(np.float32), rtol=1e-6)
    summary = M.calibration_summary({k: z[k] for k in ('totals', 'bins', 'coverages')})
    ens = {k: v for k, v in summary[-1].items()}
    want = ['calibration_' + k for k in ens] + ['calibration_n_bins', 'calibration_dropped', 'calibration_per_chain_acc', 'calibration_per_chain_brier',
                                                'calibration_per_chain_nll', 'calibration_per_chain_ece', 'calibration_per_chain_acc_median',
                                                'calibration_per_chain_brier_median', 'calibration_per_chain_nll_median',
                                                'calibration_per_chain_ece_median']
    assert sorted(k for k in m if k.startswith('calibration_')) == sorted(want)
    assert all(m['calibration_' + k] == v for k, v in ens.items())
    assert m['calibration_per_chain_nll'] == [s['nll'] for s in summary[:-1]] and m['calibration_dropped'] == 0 and m['calibration_rows'] == Nt
    assert m['calibration_coverage_0.9'] >= m['calibration_coverage_0.5'] and 1.0 <= m['calibration_set_size_0.5'] <= m['calibration_set_size_0.9'] <= K
    assert 0.0 <= m['calibration_ece'] <= m['calibration_mce'] <= 1.0
    # predict.py --sets on new rows, without labels
    table = (rng.standard_normal((20, F))).astype(np.float32)
    np.save(tmp_path / 'new.npy', table)
    _run([ROOT / 'predict.py', '-e', exp, '-i', tmp_path / 'new.npy', '-o', tmp_path / 'pred.npz', '--sets', '0.5', '0.9'])
    pred = np.load(tmp_path / 'pred.npz')
    assert sorted(pred.files) == ['class_order', 'dropped', 'entropy', 'mutual_information', 'probs', 'set_levels', 'set_size']
    assert pred['set_levels'].tolist() == [0.5, 0.9] and pred['class_order'].shape == (20, K) and pred['set_size'].shape == (20, 2)
    assert (np.sort(pred['class_order'], axis=1) == np.arange(K)).all()
    norm = np.load(exp / 'normalization.npz')
    xn = ((table - norm['x_mean']) / norm['x_std']).astype(np.float32)
    P = eng.calibration(eng.predict(torch.from_numpy(samples), torch.from_numpy(xn)), None, [0.5, 0.9])['probs'][-1].cpu().numpy()
    for n in range(20):
        cum = np.cumsum(P[n][pred['class_order'][n]])
        for q, level in enumerate((0.5, 0.9)):
            s = int(pred['set_size'][n, q])
            assert 1 <= s <= K and (cum[s - 1] >= level or s == K) and (s == 1 or cum[s - 2] < level), (n, level, s, cum)
