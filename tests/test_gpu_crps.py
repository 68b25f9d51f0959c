"""The exact CRPS of the predictive mixture on the device (mile_mixture_crps, mile_crps_stream) against tests/crps_ref.py:
given outputs over the shapes at which k_crps_pairs takes another path, contents that stress the pair term, chain weights,
non-finite draws, the streamed call on the forward kernels (bit for bit over tiles and passes), the shared workspace, the
refusals, evaluate.py --crps on a tiny run and tools/crps_time.py at a reduced size.

Error bound for given outputs, per row and per output: |got - ref| <= 1e-5 (T1 + T2 / 2), T1 = sum_c w_c a_c and T2 = w'Gw the
positive sums the output is made of (for a Gram entry: the entry).  Every pair term is >= 0 and carries about 30 fp32 roundings
(2e-6 relative: the subtraction, the sum, rsqrt, the products and the ulp bounds of the transcendentals -- erff and expf, or
the one approximation of A / s that stands in for them, 3e-7 of a term: mile_crps.hip); the fp32 run of
at most 32 terms carries as much again; 1e-5 of the positive sums bounds both.
"""
from __future__ import annotations

import ctypes as C
import json

import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import crps_ref as CR
from tests import lenetti_ref as RL
from tests.test_crps_host import BAD_SHARED
from tests.test_gpu_moments import _fcn_problem
from tests.test_gpu_predict import DEV, ROOT, _fcn_engine, _reload, _run
from tests.test_gpu_quantiles import FCN_E2E, _clip_raw, _engine, _levels

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ALL = ('crps_chain', 'spread_chain', 'crps_mix', 'spread_mix', 'gram', 'dropped')
REL = 1e-5


def _random_raw(Cn, S, N, seed):
    """[C, S, N, 2]: rows of differing centre and spread, chains offset from each other by half a spread."""
    rng = np.random.default_rng(seed)
    centre, spread = rng.standard_normal(N) * 3.0, np.exp(rng.uniform(-3.0, 1.0, N))
    mu = centre + spread * rng.standard_normal((Cn, S, N)) + 0.5 * spread * rng.standard_normal((Cn, 1, N))
    ls = rng.uniform(-2.0, 1.0, N) + 0.5 * rng.standard_normal((Cn, S, N))
    return np.stack([mu, ls], axis=-1).astype(np.float32)


def _y_near(raw, seed=11):
    rng = np.random.default_rng(seed)
    Cn, S, N = raw.shape[:3]
    pick = raw[rng.integers(0, Cn, N), rng.integers(0, S, N), np.arange(N), 0]
    return (np.nan_to_num(pick, nan=0.0, posinf=0.0, neginf=0.0) + rng.standard_normal(N).astype(np.float32)).astype(np.float32)


def _weights(Cn, seed=12):
    """uniform, a random simplex point, and the vertices e_0 and e_{C-1}"""
    w = np.random.default_rng(seed).dirichlet(np.ones(Cn))
    return np.stack([np.full(Cn, 1.0 / Cn), w / w.sum(), np.eye(Cn)[0], np.eye(Cn)[Cn - 1]])


def _bounds(ref):
    return {'crps_chain': REL * (ref['t1_chain'] + 0.5 * ref['t2_chain']), 'spread_chain': REL * (ref['t1_chain'] + 0.5 * ref['t2_chain']),
            'crps_mix': REL * (ref['t1'] + 0.5 * ref['t2']), 'spread_mix': REL * (ref['t1'] + 0.5 * ref['t2']), 'gram': REL * ref['gram']}


def _check(tag, got, ref, W):
    """got (device dict, every output) against ref within the bound, the NaN pattern, and the properties that hold exactly in
    real arithmetic.  Returns the largest achieved |got - ref| / bound."""
    g = {k: v.cpu().numpy() for k, v in got.items()}
    bounds = _bounds(ref)
    worst = 0.0
    for k, b in bounds.items():
        assert g[k].shape == ref[k].shape and g[k].dtype == np.float64, (tag, k)
        assert (np.isnan(g[k]) == np.isnan(ref[k])).all(), (tag, k, 'NaN pattern')
        fin = np.isfinite(ref[k])
        if fin.any():
            ratio = np.abs(g[k] - ref[k])[fin] / np.maximum(b[fin], 1e-300)
            worst = max(worst, float(ratio.max()))
            assert (np.abs(g[k] - ref[k])[fin] <= b[fin]).all(), (tag, k, float(ratio.max()))
    assert g['dropped'].dtype == np.int32 and (g['dropped'] == ref['dropped']).all(), tag
    assert np.array_equal(g['gram'], np.swapaxes(g['gram'], 1, 2), equal_nan=True), (tag, 'gram must be exactly symmetric')
    fin = np.isfinite(g['crps_mix'])
    assert (g['crps_mix'][fin] >= -bounds['crps_mix'][fin]).all(), (tag, 'crps >= -bound')
    finc = np.isfinite(g['crps_chain'])
    assert (g['crps_chain'][finc] >= -bounds['crps_chain'][finc]).all(), tag
    for m in range(len(W)):                                        # pooling never loses: the energy distance is >= 0
        use = W[m] != 0
        split = (W[m][use, None] * g['crps_chain'][use]).sum(axis=0)
        ok = np.isfinite(split) & np.isfinite(g['crps_mix'][1 + m])
        assert (g['crps_mix'][1 + m][ok] <= split[ok] + bounds['crps_mix'][1 + m][ok]).all(), (tag, m, 'crps_mix <= sum w crps_chain + bound')
    print(f'{tag}: max |got - ref| / bound = {worst:.4f} (bound = 1e-5 of the positive sums)')
    return worst


def _vertices(tag, got, Cn):
    """rows 3 and 4 of the mix outputs are e_0 and e_{C-1}: the chains alone, to 1e-12 relative"""
    g = {k: v.cpu().numpy() for k, v in got.items()}
    for m, c in ((3, 0), (4, Cn - 1)):
        for mix, chain in (('crps_mix', 'crps_chain'), ('spread_mix', 'spread_chain')):
            a, b = g[mix][m], g[chain][c]
            assert (np.isnan(a) == np.isnan(b)).all() and (np.abs(a - b)[np.isfinite(b)] <= 1e-12 * np.abs(b)[np.isfinite(b)]).all(), (tag, mix, c)


SHAPES = [(1, 1, 9), (3, 5, 7), (2, 257, 5), (5, 100, 70), (33, 8, 5), (1, 6000, 2)]


@pytest.mark.parametrize('Cn,S,N', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_given_outputs_over_the_shapes(Cn, S, N):
    raw = _random_raw(Cn, S, N, 1)
    y, W = _y_near(raw), _weights(Cn)
    ref = CR.crps(raw, y, W)
    got = _engine().mixture_crps(torch.from_numpy(raw), torch.from_numpy(y), weights=W, outputs=ALL)
    assert not got['dropped'].any()
    _check(f'{Cn}x{S}x{N}', got, ref, W)
    _vertices(f'{Cn}x{S}x{N}', got, Cn)
    if (Cn, S) == (1, 1):                                           # one Normal: the closed form
        exact = CR.single_normal_crps(raw[0, 0, :, 0].astype(np.float64), np.exp(raw[0, 0, :, 1].astype(np.float64)), y)
        sig = np.exp(raw[0, 0, :, 1].astype(np.float64))
        t1 = CR.abs_normal_mean(y.astype(np.float64) - raw[0, 0, :, 0], sig ** 2)
        assert (np.abs(got['crps_mix'][0].cpu().numpy() - exact) <= REL * (t1 + sig / np.sqrt(np.pi))).all()
    if (Cn, S, N) == (5, 100, 70):                                  # every row tiling, and fewer outputs: the same bits
        for rows in (1, 32, 33):
            again = _engine().mixture_crps(torch.from_numpy(raw), torch.from_numpy(y), weights=W, outputs=ALL, max_rows_per_tile=rows)
            assert all(torch.equal(again[k], got[k]) for k in ALL), rows
        only = _engine().mixture_crps(torch.from_numpy(raw), torch.from_numpy(y), outputs=('crps_mix',))
        assert list(only) == ['crps_mix'] and torch.equal(only['crps_mix'][0], got['crps_mix'][0])
        drop = _engine().mixture_crps(torch.from_numpy(raw), torch.from_numpy(y), outputs=('dropped',))
        assert list(drop) == ['dropped'] and not drop['dropped'].any()


def _clips():
    a, b = _clip_raw(), _clip_raw()[::-1]                           # [64, 6, 2] each: log sigma at and beyond both clips
    return np.ascontiguousarray(np.stack([a, b]))


def _identical():
    raw = np.empty((2, 40, 3, 2), dtype=np.float32)
    raw[..., 0] = np.array([0.0, -3.25, 1e3], dtype=np.float32)
    raw[..., 1] = np.array([0.0, -2.0, 3.0], dtype=np.float32)
    return raw


def _far_groups():
    """sigma = 1 and groups 1e8 apart, inside the chains and between them: A = |delta| to fp32"""
    rng = np.random.default_rng(7)
    raw = np.zeros((3, 50, 4, 2), dtype=np.float32)
    raw[..., 0] = rng.standard_normal((3, 50, 4))
    raw[0, ::2, :, 0] += 1e8
    raw[1, :, 1:, 0] += 1e8
    raw[2, :10, :, 0] -= 1e8
    return raw


def _sharp():
    """mu within 1e-3 of 100, sigma at the lower clip, y = 100.0005: T1 and T2 / 2 are of one size, a thousand sigma each, and
    every delta is a difference of two fp32 values near 100"""
    rng = np.random.default_rng(8)
    raw = np.empty((2, 300, 4, 2), dtype=np.float32)
    raw[..., 0] = 100.0 + 1e-3 * rng.uniform(-1.0, 1.0, (2, 300, 4))
    raw[..., 1] = np.log(1e-6)
    return raw


CONTENT = {'sigma_clips': _clips, 'identical_draws': _identical, 'far_groups': _far_groups, 'sharp': _sharp}


@pytest.mark.parametrize('case', list(CONTENT))
def test_given_outputs_by_content(case):
    raw = CONTENT[case]()
    Cn, _, N = raw.shape[:3]
    y = np.full(N, 100.0005, dtype=np.float32) if case == 'sharp' else _y_near(raw)
    W = _weights(Cn)
    ref = CR.crps(raw, y, W)
    got = _engine().mixture_crps(torch.from_numpy(raw), torch.from_numpy(y), weights=W, outputs=ALL)
    _check(case, got, ref, W)
    _vertices(case, got, Cn)
    if case == 'sharp':
        r = ref['t1'][0] / (0.5 * ref['t2'][0])
        print(f'sharp: T1 / (T2 / 2) from {r.min():.4f} to {r.max():.4f}, crps {ref["crps_mix"][0].min():.3e} .. {ref["crps_mix"][0].max():.3e}')


def test_nonfinite_draws_are_left_out_per_row():
    raw = _random_raw(3, 50, 6, 9)
    raw[0, 3, 0, 0] = np.nan
    raw[0, 4, 0, 1] = np.inf
    raw[1, 5, 1, 0] = -np.inf
    raw[2, 7, 1, 1] = -np.inf
    raw[2, 9, 1, 1] = np.nan
    raw[:, :, 2, 0] = np.nan                                        # nothing kept on row 2
    raw[1, :, 3, 1] = np.inf                                        # chain 1 wholly dropped on row 3
    raw[0, 1:, 4, 0] = np.nan                                       # one draw of chain 0 kept on row 4
    y = _y_near(raw)
    W = np.stack([np.full(3, 1.0 / 3.0), [0.5, 0.0, 0.5], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    ref = CR.crps(raw, y, W)
    got = _engine().mixture_crps(torch.from_numpy(raw), torch.from_numpy(y), weights=W, outputs=ALL)
    assert got['dropped'].tolist() == [[2, 0, 50, 0, 49, 0], [0, 1, 50, 50, 0, 0], [0, 2, 50, 0, 0, 0]]
    _check('nonfinite', got, ref, W)
    g = {k: v.cpu().numpy() for k, v in got.items()}
    assert np.isnan(g['crps_mix'][:, 2]).all() and np.isnan(g['crps_chain'][:, 2]).all() and np.isnan(g['gram'][2]).all()
    assert np.isnan(g['crps_chain'][1, 3]) and np.isnan(g['gram'][3, 1]).all() and np.isnan(g['gram'][3, :, 1]).all()
    assert np.isfinite(g['crps_mix'][0, 3]) and np.isnan(g['crps_mix'][1, 3]) and np.isfinite(g['crps_mix'][2, 3])    # pooled and w_1 = 0 skip it
    # the pooled weights are K_c / sum K: row 4 keeps 1, 50 and 50 draws
    np.testing.assert_allclose(ref['pooled'][4], [1 / 101, 50 / 101, 50 / 101], rtol=1e-15)
    w4 = np.array([[1 / 101, 50 / 101, 50 / 101]])
    w4 /= w4.sum()
    own = _engine().mixture_crps(torch.from_numpy(raw), torch.from_numpy(y), weights=w4, outputs=('crps_mix',))['crps_mix'].cpu().numpy()
    assert abs(own[1, 4] - own[0, 4]) <= 1e-12 * ref['t1'][0, 4]
    # the kept draws alone give the same numbers: a left-out draw has weight 0
    keep = np.isfinite(raw[0, :, 0]).all(axis=-1)
    sub = np.ascontiguousarray(raw[:1, keep, :1])
    alone = _engine().mixture_crps(torch.from_numpy(sub), torch.from_numpy(y[:1]), outputs=('crps_chain',))['crps_chain'].cpu().numpy()
    assert abs(alone[0, 0] - g['crps_chain'][0, 0]) <= 2 * REL * (ref['t1_chain'][0, 0] + 0.5 * ref['t2_chain'][0, 0])


# ---- streamed ---------------------------------------------------------------------------------------------------------------
def _sigma(ls):
    with np.errstate(over='ignore'):
        return np.clip(np.exp(ls.astype(np.float64)), 1e-6, 1e6)


def _streamed(tag, eng, theta, X, out64, Cn):
    """theta [C * S, d] as C chains: bitwise mixture_crps(predict), bitwise over tiles and passes, and crps_ref on the fp64
    forwards within 2 max|d mu| + 1.6 max|d sigma| + the 1e-5 term (A is 1-Lipschitz in delta, sqrt(2 / pi)-Lipschitz in s)."""
    D, N = out64.shape[:2]
    S = D // Cn
    samples = torch.from_numpy(theta).reshape(Cn, S, -1)
    Xt = torch.from_numpy(X)
    ref_mu = out64[..., 0]
    y = (ref_mu[np.random.default_rng(12).integers(0, D, N), np.arange(N)] + 0.3 * np.random.default_rng(13).standard_normal(N)).astype(np.float32)
    yt, W = torch.from_numpy(y), _weights(Cn)
    base = eng.crps_stream(samples, Xt, yt, weights=W, outputs=ALL)
    raw = eng.predict(samples, Xt)
    alone = eng.mixture_crps(raw, yt, weights=W, outputs=ALL)
    assert all(torch.equal(alone[k], base[k]) for k in ALL), (tag, 'crps_stream != mixture_crps(predict)')
    for rows in (0, 1, 32, 33):
        for draws in (0, 1, 7, S):
            if (rows, draws) == (0, 0):
                continue
            got = eng.crps_stream(samples, Xt, yt, weights=W, outputs=ALL, max_rows_per_tile=rows, max_draws_per_pass=draws)
            assert all(torch.equal(got[k], base[k]) for k in ALL), (tag, rows, draws)
    r32 = raw.cpu().numpy().reshape(D, N, 2)
    d_mu = float(np.abs(r32[..., 0].astype(np.float64) - out64[..., 0]).max())
    d_sig = float(np.abs(_sigma(r32[..., 1]) - _sigma(out64[..., 1])).max())
    ref = CR.crps(out64.reshape(Cn, S, N, 2), y, W)
    slack = 2.0 * d_mu + 1.6 * d_sig
    g = {k: v.cpu().numpy() for k, v in base.items()}
    for k, b in _bounds(ref).items():
        err = np.abs(g[k] - ref[k])
        print(f'{tag} {k}: max err {err.max():.3e}, bound {float((slack + b).min()):.3e} .. (forward: max|d mu| {d_mu:.2e}, max|d sigma| {d_sig:.2e})')
        assert (err <= slack + b).all(), (tag, k, float(err.max()), slack)
    assert not base['dropped'].any()


@pytest.mark.parametrize('kernel,hs', FCN_E2E)
def test_fcn_streamed(kernel, hs):
    ospec, prob, X = _fcn_problem(5, hs, 'relu', 'regr', 70, 300)
    eng = _fcn_engine(ospec, prob, kernel)
    _streamed(kernel, eng, prob['theta0'], X, O.mlp_forward(ospec, prob['theta0'].astype(np.float64), X.astype(np.float64)), 3)


def test_lenetti_streamed():
    from mile_amd import LeNettiSpec
    from mile_amd.engine import Engine
    ospec = RL.LeNettiSpec(3, 9, 11, 2, activation='tanh', task='regr')
    prob = RL.synthetic_problem(ospec, 20, 6, seed=6)
    X = RL.synthetic_problem(ospec, 70, 1, seed=7)['X']
    eng = Engine(LeNettiSpec(3, 9, 11, 2, activation='tanh', task='regr'), torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV)
    assert eng.grad_kernel == 'lenetti_f32'
    _streamed('lenetti', eng, prob['theta0'], X.reshape(len(X), -1), RL.forward(ospec, prob['theta0'].astype(np.float64), X), 2)


def test_streamed_calls_share_one_workspace():
    eng = _engine()
    ospec, prob, X = _fcn_problem(5, (16, 16, 2), 'relu', 'regr', 70, 12)
    th, Xt, levels = torch.from_numpy(prob['theta0']), torch.from_numpy(X), _levels()
    y = torch.from_numpy(np.random.default_rng(13).standard_normal(70).astype(np.float32))
    first = eng.predict_quantiles(th, Xt, levels, y=y, return_dropped=True)
    assert eng.debug_quantile_sweeps()[0] == 70
    res = eng.crps_stream(th.reshape(3, 4, -1), Xt, y)
    assert eng.debug_quantile_sweeps()[0] == 0                      # the sweeps lay in the buffer crps_stream has reused
    again = eng.predict_quantiles(th, Xt, levels, y=y, return_dropped=True)
    assert all(torch.equal(a, b) for a, b in zip(again, first))
    assert torch.isfinite(res['crps_mix']).all() and eng.crps_stream_workspace(3, 4, 70) > 0


def test_refusals_leave_the_handle_usable():
    ospec, prob, X = _fcn_problem(5, (16, 16, 2), 'relu', 'regr', 70, 24)
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    samples, Xt = torch.from_numpy(prob['theta0']).reshape(3, 8, -1).to(DEV), torch.from_numpy(X).to(DEV)
    y = torch.zeros(70, device=DEV)
    out = torch.full((70 * 9 * 9,), 7.0, dtype=torch.float64, device=DEV)
    raw = eng.predict(samples, Xt)
    p = lambda t: C.c_void_p(t.data_ptr())
    o = p(out)

    def stream(h=eng._h, theta=p(samples), Cn=3, S=8, Xp=p(Xt), yp=p(y), N=70, w=None, n_w=0, outs=(o,) * 6, passes=0, tile=0):
        return eng.lib.mile_crps_stream(h, theta, Cn, S, Xp, yp, N, w, n_w, *outs, passes, tile, None)

    def given(rawp=p(raw), Cn=3, S=8, N=70, yp=p(y), w=None, n_w=0, outs=(o,) * 6, tile=0):
        return eng.lib.mile_mixture_crps(rawp, Cn, S, N, yp, w, n_w, *outs, tile, None)
    for tag, kw, text in [('null handle', dict(h=None), 'null'), ('null theta', dict(theta=None), 'null'), ('null X', dict(Xp=None), 'null'),
                          ('null y', dict(yp=None), 'null'), ('passes < 0', dict(passes=-1), 'max_draws_per_pass')] + BAD_SHARED:
        assert stream(**kw) == -1, tag
        assert text in eng.lib.mile_last_error().decode(), tag
    for tag, kw, text in [('null raw', dict(rawp=None), 'null'), ('null y', dict(yp=None), 'null')] + BAD_SHARED:
        assert given(**kw) == -1, tag
        assert text in eng.lib.mile_last_error().decode(), tag
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                 # nothing was launched
    cspec, cprob, cX = _fcn_problem(7, (40, 40, 3), 'tanh', 'classification', 30, 4)
    ceng = _fcn_engine(cspec, cprob, 'mfma_narrow_f32')
    cs, cXt = torch.from_numpy(cprob['theta0']).reshape(2, 2, -1).to(DEV), torch.from_numpy(cX).to(DEV)
    assert eng.lib.mile_crps_stream(ceng._h, p(cs), 2, 2, p(cXt), p(y), 30, None, 0, *(o,) * 6, 0, 0, None) == -1
    assert 'regression' in eng.lib.mile_last_error().decode()
    with pytest.raises(ValueError):
        ceng.crps_stream(cs, cXt, y[:30])
    with pytest.raises(ValueError):
        eng.crps_stream(samples, Xt, y, weights=[0.5, 0.6, -0.1])
    with pytest.raises(ValueError):
        eng.crps_stream(samples, Xt, y, outputs=())
    assert torch.isfinite(ceng.predict(cs, cXt)).all()              # both handles go on working
    res = eng.crps_stream(samples, Xt, y, weights=[0.5, 0.25, 0.25])
    assert torch.isfinite(res['crps_mix']).all() and res['crps_mix'].shape == (2, 70)
    assert eng.crps_stream_workspace(0, 8, 70) == -1 and eng.crps_stream_workspace(3, 8, 0) == -1


# ---- command line -----------------------------------------------------------------------------------------------------------
def test_evaluate_cli_crps(tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=120, n_chains=4)      # thinning 10: 12 draws kept per chain
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    _run([ROOT / 'train.py', '-c', tmp_path / 'cfg.yaml', '-d', '1'])
    exp = tmp_path / 'smoke_synthetic'
    _run([ROOT / 'evaluate.py', '-e', exp, '--crps'])
    m = json.loads((exp / 'metrics.json').read_text())
    plain = {k: v for k, v in m.items() if not k.startswith('crps')}
    names = ('', '_se', '_spread', '_spread_se', '_uniform', '_uniform_se', '_uniform_pooling_gain', '_per_chain', '_per_chain_median',
             '_per_chain_spread', '_rows_nan', '_thin_stride', '_dropped', '_energy_distance_max')
    assert sorted(k for k in m if k.startswith('crps')) == sorted('crps' + k for k in names)
    z = np.load(exp / 'crps.npz')
    n = plain['n_points']
    assert sorted(z.files) == sorted(ALL + ('energy_distance', 'weights', 'thin_stride'))
    assert z['crps_chain'].shape == z['spread_chain'].shape == z['dropped'].shape == (4, n) and z['crps_mix'].shape == z['spread_mix'].shape == (2, n)
    assert z['gram'].shape == (n, 4, 4) and z['energy_distance'].shape == (4, 4) and int(z['thin_stride']) == 1 == m['crps_thin_stride']
    assert m['crps'] > 0 and m['crps_spread'] > 0 and m['crps_uniform'] == pytest.approx(m['crps'], rel=1e-9) and m['crps_dropped'] == 0
    assert m['crps_uniform_pooling_gain'] >= -1e-5 * (m['crps'] + m['crps_spread']) and len(m['crps_per_chain']) == 4
    _run([ROOT / 'evaluate.py', '-e', exp, '--crps', '--stacking', '--crps-max-draws', '24'])
    m2 = json.loads((exp / 'metrics.json').read_text())
    assert {k: v for k, v in m2.items() if not k.startswith(('crps', 'stacking'))} == plain      # every other key as it was
    z2, w = np.load(exp / 'crps.npz'), np.load(exp / 'stacking.npz')['weights']
    assert {'crps_stacked', 'crps_stacked_se', 'crps_stacked_pooling_gain'} <= set(m2) and m2['crps_thin_stride'] == 2 == int(z2['thin_stride'])
    assert z2['crps_mix'].shape == (3, n) and z2['weights'].shape == (2, 4) and np.abs(z2['weights'][1] - w).max() <= 1e-12
    eng, samples, x, y = _reload(exp, 'test')
    res = eng.crps_stream(torch.from_numpy(np.ascontiguousarray(samples[:, ::2])), torch.from_numpy(x), torch.from_numpy(y), weights=z2['weights'][1],
                          outputs=('crps_mix',))['crps_mix'].cpu().numpy()
    assert np.array_equal(res[1], z2['crps_mix'][2]) and np.array_equal(res[0], z2['crps_mix'][0])
    assert m2['crps_stacked'] == pytest.approx(float(res[1].mean()), rel=1e-12)
    print(f"cli: crps {m2['crps']:.6f}, crps_uniform {m2['crps_uniform']:.6f}, crps_stacked {m2['crps_stacked']:.6f}, weights {w}")


def test_the_timing_tool_at_a_reduced_size():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, str(ROOT / 'tools' / 'crps_time.py'), '--shapes', 'tiny', '--reps', '1', '--valu-per-pair', '39'],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec['shape'] == 'tiny' and rec['pairs'] == 120 * 121 // 2 * 17 and rec['pairs_per_s'] > 0 and rec['dense_rows'] == 17
    assert max(rec[f'max_rel_diff_{k}'] for k in ('crps_chain', 'crps_mix', 'spread_mix')) < 1e-5
