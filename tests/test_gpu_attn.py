"""AttentionClassifier on its HIP kernel (k_grad_attn / k_fwd_attn) vs the fp64 restatement tests/attn_ref.py (-m gpu)."""
import numpy as np
import pytest

from tests import attn_ref as R
from tests import nuts_ref as NR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


def _spec(V, T, C, H, D, K=2, proj=(32,), bias=False, prior='Normal', scale=0.2):
    from mile_amd.spec import AttentionSpec
    return AttentionSpec(V, T, C, H, D, n_classes=K, projection_dim=proj, use_bias=bias, prior=prior, prior_scale=scale)


def _engine(spec, X, y):
    from mile_amd.engine import Engine
    eng = Engine(spec, torch.from_numpy(X), torch.from_numpy(y), device='cuda:0')
    assert eng.grad_kernel == 'attn_f32'
    return eng


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _check(lp, g, lp_ref, g_ref):
    """DESIGN section 1 tolerances: log-density 2e-5 relative, gradient 2e-5 of its largest entry (per chain)."""
    lp, g = lp.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    assert np.abs(lp - lp_ref).max() < 2e-5 * max(1.0, np.abs(lp_ref).max()), (lp, lp_ref)
    for e in range(g.shape[0]):
        err = np.abs(g[e] - g_ref[e])
        assert err.max() < 2e-5 * np.abs(g_ref[e]).max(), (e, int(err.argmax()), err.max(), np.abs(g_ref[e]).max())


CASES = [
    # V, T, C, H, D, K, proj, bias, N, E
    (1000, 70, 48, 8, 64, 2, (32,), False, 64, 3),       # sequential_mod.yaml's shape
    (50, 37, 24, 4, 32, 3, (20, 12), True, 41, 2),       # bias, two projections, K = 3, T = 37
    (30, 20, 32, 2, 32, 2, (16,), False, 9, 2),          # hd = 16
    (30, 16, 64, 1, 64, 4, (8,), True, 7, 2),            # hd = 64: dK in LDS
    (17, 11, 8, 2, 8, 2, (), True, 1, 1),                # N = 1, E = 1, no projection
    (200, 128, 64, 8, 64, 16, (64, 64), True, 5, 2),     # widest supported
    (60, 128, 64, 2, 64, 2, (16,), False, 6, 2),         # hd = 32 at T = 128: dK in LDS, two 16-column tiles per key tile
]
# the ceil(hd / 16) instantiations of the shared attention backward that CASES does not reach.  A list of its own: tests/leaf_cases.py
# builds its sharp problems from CASES, and their ids count its entries
NHT_CASES = [
    (30, 16, 16, 1, 48, 2, (8,), True, 5, 2),            # hd = 48: three 16-column dK / dq tiles
]


@pytest.mark.parametrize('V,T,C,H,D,K,proj,bias,N,E', CASES + NHT_CASES)
def test_logpost_grad_matches_restatement(V, T, C, H, D, K, proj, bias, N, E):
    spec = _spec(V, T, C, H, D, K, proj, bias)
    prob = R.synthetic_problem(spec, N, E, seed=3)
    lp_ref, g_ref = R.logpost_and_grad(spec, prob['theta0'], prob['x'], prob['y'])
    eng = _engine(spec, prob['X'], prob['y'])
    lp, g = eng.logpost_grad(torch.from_numpy(prob['theta0']))
    torch.cuda.synchronize()
    _check(lp, g, lp_ref, g_ref)
    assert eng.grad_launch_info(E)['lds_bytes'] == spec.lds_bytes


def test_row_splits_and_windows():
    """Ensembles of 1, 2 and 4 chains split the rows into different ranges; a row window gives what a fresh engine on those
    rows gives and what the restatement gives on them."""
    spec = _spec(300, 24, 32, 4, 32, 2, (16,), True)
    N = 600
    prob = R.synthetic_problem(spec, N, 2, seed=4)
    lp_ref, g_ref = R.logpost_and_grad(spec, prob['theta0'], prob['x'], prob['y'])
    eng = _engine(spec, prob['X'], prob['y'])
    th = torch.from_numpy(prob['theta0'])
    _check(*eng.logpost_grad(th), lp_ref, g_ref)
    _check(*eng.logpost_grad(th[:1]), lp_ref[:1], g_ref[:1])
    lp4, g4 = eng.logpost_grad(th.repeat(2, 1))
    _check(lp4, g4, np.tile(lp_ref, 2), np.tile(g_ref, (2, 1)))
    b, c = 100, 77
    eng.set_row_window(b, c)
    lpw, gw = eng.logpost_grad(th)
    eng.set_row_window(0, 0)
    fresh = _engine(spec, np.ascontiguousarray(prob['X'][b:b + c]), np.ascontiguousarray(prob['y'][b:b + c]))
    lpf, gf = fresh.logpost_grad(th)
    assert _relerr(lpw.cpu().numpy(), lpf.cpu().numpy()) < 1e-6 and _relerr(gw.cpu().numpy(), gf.cpu().numpy()) < 1e-5
    lpr, gr = R.logpost_and_grad(spec, prob['theta0'], prob['x'][b:b + c], prob['y'][b:b + c])
    _check(lpw, gw, lpr, gr)


def test_warmstart_steps_match_the_optax_rules():
    """mile_warmstart_step on row windows (likelihood gradient + one fused adamw launch, in place) against the host-side
    restatement of optax's rules (`warmstart._Optimizer`) driven by attn_ref's gradient of the window's mean negative
    log-likelihood: four steps over two windows, one member frozen -- parameters, moments and the reported batch NLL."""
    from mile_amd.warmstart import _Optimizer
    spec = _spec(80, 20, 16, 4, 16, 2, (8,), True)
    E, N, bs = 3, 64, 32
    prob = R.synthetic_problem(spec, N, E, seed=17)
    eng = _engine(spec, prob['X'], prob['y'])
    params = {'learning_rate': 0.01, 'weight_decay': 0.001}
    th_a = torch.from_numpy(prob['theta0']).cuda().contiguous()
    th_b = torch.from_numpy(prob['theta0']).clone()
    ref = _Optimizer('adamw', params, th_b)
    ost = {'name': 'adamw', 'learning_rate': ref.lr, 'b1': ref.b1, 'b2': ref.b2, 'eps': ref.eps, 'weight_decay': ref.wd,
           't': 0, 'm': torch.zeros_like(th_a), 'v': torch.zeros_like(th_a)}
    active = torch.tensor([True, False, True])
    for k in range(4):
        r0 = (k % 2) * bs
        eng.set_row_window(r0, bs)
        nll_a = eng.warmstart_step(th_a, ost, active.cuda(), want_nll=True)
        lg = [R.loglik_and_grad(spec, t, prob['x'][r0:r0 + bs], prob['y'][r0:r0 + bs]) for t in th_b.numpy().astype(np.float64)]
        nll_b = -np.array([ll for ll, _ in lg]) / bs
        gl = np.stack([g for _, g in lg])
        th_b = ref.step(th_b, torch.from_numpy((-gl / bs).astype(np.float32)), active)
        assert _relerr(nll_a[active.cuda()].cpu().numpy(), nll_b[active.numpy()]) < 1e-4, k
    eng.set_row_window(0, 0)
    torch.cuda.synchronize()
    assert torch.equal(th_a[1].cpu(), torch.from_numpy(prob['theta0'][1]))          # frozen member untouched
    # adamw divides by sqrt(v) + eps: entries whose gradient is rounding-sized move by O(lr) whatever the rounding is
    # (tests/test_gpu_e2e.py's FCN form of this check explains and measures it), so parameters get 5e-4, moments 1e-4
    assert _relerr(th_a.cpu().numpy(), th_b.numpy()) < 5e-4
    assert _relerr(ost['m'].cpu().numpy(), ref.m.numpy()) < 1e-4 and _relerr(ost['v'].cpu().numpy(), ref.v.numpy()) < 1e-4
    assert ost['m'][1].abs().max().item() == 0.0 and ost['t'] == 4


def test_pointwise_loglik_matches_restatement():
    spec = _spec(100, 30, 16, 4, 16, 3, (8,), True)
    prob = R.synthetic_problem(spec, 20, 5, seed=6)
    test = R.synthetic_problem(spec, 301, 1, seed=7)
    eng = _engine(spec, prob['X'], prob['y'])
    pw = eng.pointwise_loglik(torch.from_numpy(prob['theta0']), torch.from_numpy(test['X']), torch.from_numpy(test['y']))
    ref = np.stack([R.pointwise_loglik(spec, t, test['x'], test['y']) for t in prob['theta0']])
    assert pw.shape == (5, 301)
    assert np.abs(pw.cpu().numpy() - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())


def test_token_ids_validated():
    spec = _spec(10, 8, 8, 2, 8, 2, (4,))
    prob = R.synthetic_problem(spec, 4, 1, seed=1)
    X = prob['X'].copy()
    X[0, 0] = 10
    with pytest.raises(ValueError):
        _engine(spec, X, prob['y'])


def test_mclmc_steps_match_oracle(oracle):
    spec = _spec(40, 12, 16, 4, 16, 2, (8,), False)
    N, E, T = 48, 3, 4
    prob = R.synthetic_problem(spec, N, E, seed=9)
    rng = np.random.default_rng(4)
    d = spec.n_params
    z0 = rng.standard_normal((E, d)).astype(np.float32)
    noise = rng.standard_normal((T, 2, E, d)).astype(np.float32)
    f = lambda th: R.logpost_and_grad(spec, th, prob['x'], prob['y'])     # noqa: E731
    st = oracle.mclmc_init(f, prob['theta0'].astype(np.float64), z0.astype(np.float64))
    for i in range(T):
        st, info = oracle.mclmc_step(f, st, prob['eps'].astype(np.float64), prob['L'].astype(np.float64),
                                     noise[i, 0].astype(np.float64), noise[i, 1].astype(np.float64))
    eng = _engine(spec, prob['X'], prob['y'])
    s = eng.init(torch.from_numpy(prob['theta0']), noise=torch.from_numpy(z0))
    s, info_g, _ = eng.step(s, torch.from_numpy(prob['eps']), torch.from_numpy(prob['L']), n_steps=T, noise=torch.from_numpy(noise))
    torch.cuda.synchronize()
    assert _relerr(s.position.cpu().numpy(), st.position) < 1e-4
    assert _relerr(s.logdensity.cpu().numpy(), st.logdensity) < 1e-5
    assert _relerr(s.logdensity_grad.cpu().numpy(), st.logdensity_grad) < 1e-3
    assert np.abs(info_g.energy_change[-1].cpu().numpy() - info.energy_change).max() < 5e-3


def test_nuts_step_teacher_forced():
    spec = _spec(30, 10, 8, 2, 8, 2, (8,), True)
    N, E, M, eps = 30, 3, 5, 0.01
    prob = R.synthetic_problem(spec, N, E, seed=12)
    d = spec.n_params
    rng = np.random.default_rng(12)
    z = rng.standard_normal((1, E, d)).astype(np.float32)
    u = rng.uniform(size=(1, E, 2 * M + 2 ** M)).astype(np.float32)
    m = rng.uniform(0.5, 1.5, (E, d)).astype(np.float32)

    def f(x):
        lp, g = R.logpost_and_grad(spec, np.asarray(x, np.float64)[None], prob['x'], prob['y'])
        return float(lp[0]), g[0]

    eng = _engine(spec, prob['X'], prob['y'])
    s0 = eng.nuts_init(torch.from_numpy(prob['theta0']))
    s1, info, _ = eng.nuts_step(s0, torch.full((E,), eps), torch.from_numpy(m), max_num_doublings=M, noise=torch.from_numpy(z),
                                uniforms=torch.from_numpy(u))
    torch.cuda.synchronize()
    got = np.stack([t[0].cpu().numpy() for t in info], axis=1)
    for e in range(E):
        x = prob['theta0'][e].astype(np.float64)
        lp, g = f(x)
        st, inf = NR.nuts_step(f, NR.HMCState(x, lp, g), float(np.float32(eps)), m[e].astype(np.float64), z[0, e].astype(np.float64),
                               u[0, e].astype(np.float64), M)
        want = (inf.num_integration_steps, inf.num_trajectory_expansions, inf.is_divergent, inf.is_turning)
        assert tuple(int(v) for v in got[e, [0, 2, 3, 5]]) == tuple(int(v) for v in want), (e, got[e], inf)
        assert _relerr(s1.position[e].cpu().numpy(), st.position) < 1e-3, e


def test_train_and_evaluate_cli(tmp_path):
    """`train.py -c` on a shrunken copy of experiments/mclmc_seqmod_synthetic.yaml (warm start on row windows, 30 + 20 MCLMC
    steps), then `evaluate.py`."""
    import json
    import subprocess
    import sys
    from pathlib import Path

    import yaml
    root = Path(__file__).resolve().parents[1]
    cfg = yaml.safe_load((root / 'experiments' / 'mclmc_seqmod_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['experiment_name'] = 'seqmod_small'
    cfg['data']['path'] = '400x20x50'
    cfg['data']['datapoint_limit'] = 400
    cfg['model'].update(context_len=20, vocab_size=50)
    cfg['training']['warmstart'].update(max_epochs=3, patience=2)
    cfg['training']['sampler'].update(warmup_steps=30, n_samples=20, n_chains=3, n_thinning=10)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, str(root / 'train.py'), '-c', str(tmp_path / 'cfg.yaml'), '-d', '1'],
                       capture_output=True, text=True, cwd=root, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp = tmp_path / 'seqmod_small'
    assert 'Warmstart Training completed' in (exp / 'training.log').read_text()
    assert sorted(p.name for p in (exp / 'samples').iterdir() if p.is_dir()) == ['0', '1', '2']
    z = np.load(exp / 'samples' / '2' / 'sample_10.npz')
    assert z.files == ['MDPA.key.kernel', 'MDPA.out.kernel', 'MDPA.query.kernel', 'MDPA.value.kernel',
                       'TokenEmbedding_0.Embedding.embedding', 'TokenEmbedding_0.PositionEmbedding.embedding',
                       'classifier.kernel', 'projection_0.kernel']
    assert z['MDPA.key.kernel'].shape == (48, 8, 8) and z['MDPA.out.kernel'].shape == (8, 8, 48)
    assert z['TokenEmbedding_0.Embedding.embedding'].shape == (50, 48)
    assert all(np.isfinite(z[k]).all() for k in z.files)
    r = subprocess.run([sys.executable, str(root / 'evaluate.py'), '-e', str(exp), '--split', 'valid'], capture_output=True,
                       text=True, cwd=root, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = json.loads((exp / 'metrics.json').read_text())
    assert m['split'] == 'valid' and m['n_points'] == 40 and np.isfinite(m['lppd'])
