"""PretrainedAttentionClassifier on its HIP kernel (k_grad_attn_pre / k_fwd_attn_pre) vs the fp64 restatement
tests/attn_pre_ref.py (-m gpu)."""
import numpy as np
import pytest

from tests import attn_pre_ref as R
from tests import nuts_ref as NR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


def _spec(V, T, C, H, D, K=2, proj=(32,), bias=True, prior='Normal', scale=0.2):
    from mile_amd.spec import PretrainedAttentionSpec
    return PretrainedAttentionSpec(V, T, C, H, D, n_classes=K, projection_dim=proj, use_bias=bias, prior=prior, prior_scale=scale)


def _engine(spec, prob, X=None, y=None):
    from mile_amd.engine import Engine
    X = prob['X'] if X is None else X
    y = prob['y'] if y is None else y
    eng = Engine(spec, torch.from_numpy(X), torch.from_numpy(y), device='cuda:0', tables=(prob['emb'], prob['pos']))
    assert eng.grad_kernel == 'attn_pre_f32'
    return eng


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _ref(spec, prob, theta=None, x=None, y=None):
    return R.logpost_and_grad(spec, prob['theta0'] if theta is None else theta, prob['emb'], prob['pos'],
                              prob['x'] if x is None else x, prob['y'] if y is None else y)


def _check(lp, g, lp_ref, g_ref):
    """DESIGN section 1 tolerances: log-density 2e-5 relative, gradient 2e-5 of its largest entry (per chain)."""
    lp, g = lp.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    assert np.abs(lp - lp_ref).max() < 2e-5 * max(1.0, np.abs(lp_ref).max()), (lp, lp_ref)
    for e in range(g.shape[0]):
        err = np.abs(g[e] - g_ref[e])
        assert err.max() < 2e-5 * np.abs(g_ref[e]).max(), (e, int(err.argmax()), err.max(), np.abs(g_ref[e]).max())


CASES = [
    # V, T, C, H, D, K, proj, bias, N, E
    (10000, 70, 192, 8, 64, 2, (32,), True, 24, 2),          # sequential_mod_pretrained.yaml (hd = 8)
    (10000, 70, 192, 10, 100, 2, (128, 32), True, 20, 2),    # sequential_mod_pretrained_larger.yaml (hd = 10)
    (300, 37, 61, 2, 32, 3, (20,), False, 17, 2),            # C, T not multiples of 16, hd = 16, K = 3, no bias
    (200, 50, 100, 2, 64, 2, (), True, 9, 3),                # hd = 32 (dK in LDS), no projection
    (50, 16, 24, 1, 100, 2, (128, 8), False, 5, 1),          # one head of 100 (seven dq tiles)
    (80, 128, 64, 4, 64, 16, (16,), True, 4, 2),             # T = 128, K = 16
]
# the ceil(hd / 16) instantiations of the shared attention backward that CASES does not reach.  A list of its own: tests/leaf_cases.py
# builds its sharp problems from CASES, and their ids count its entries
NHT_CASES = [
    (40, 20, 24, 2, 96, 2, (8,), True, 5, 2),                # hd = 48: three dq tiles
    (40, 20, 24, 1, 64, 2, (8,), True, 5, 2),                # hd = 64: four
    (40, 20, 24, 1, 80, 2, (8,), True, 5, 2),                # hd = 80: five
    (40, 20, 24, 1, 96, 2, (8,), True, 5, 2),                # hd = 96: six
    (40, 20, 24, 1, 128, 2, (8,), True, 5, 2),               # hd = 128: eight, the most
]


@pytest.mark.parametrize('V,T,C,H,D,K,proj,bias,N,E', CASES + NHT_CASES)
def test_logpost_grad_matches_restatement(V, T, C, H, D, K, proj, bias, N, E):
    spec = _spec(V, T, C, H, D, K, proj, bias)
    prob = R.synthetic_problem(spec, N, E, seed=3)
    eng = _engine(spec, prob)
    lp, g = eng.logpost_grad(torch.from_numpy(prob['theta0']))
    torch.cuda.synchronize()
    _check(lp, g, *_ref(spec, prob))
    assert eng.grad_launch_info(E)['lds_bytes'] == spec.lds_bytes
    assert eng.grad_launch_info(E)['kernel'] == 'k_grad_attn_pre'


def test_row_splits_and_windows():
    """Ensembles of 1, 2 and 4 chains split the rows into different ranges (some of them empty); a row window gives what a
    fresh engine on those rows gives and what the restatement gives on them."""
    spec = _spec(300, 24, 40, 4, 32, 2, (16,), True)
    N = 600
    prob = R.synthetic_problem(spec, N, 2, seed=4)
    lp_ref, g_ref = _ref(spec, prob)
    eng = _engine(spec, prob)
    th = torch.from_numpy(prob['theta0'])
    _check(*eng.logpost_grad(th), lp_ref, g_ref)
    _check(*eng.logpost_grad(th[:1]), lp_ref[:1], g_ref[:1])
    _check(*eng.logpost_grad(th.repeat(2, 1)), np.tile(lp_ref, 2), np.tile(g_ref, (2, 1)))
    b, c = 100, 77
    eng.set_row_window(b, c)
    lpw, gw = eng.logpost_grad(th)
    eng.set_row_window(0, 0)
    fresh = _engine(spec, prob, np.ascontiguousarray(prob['X'][b:b + c]), np.ascontiguousarray(prob['y'][b:b + c]))
    lpf, gf = fresh.logpost_grad(th)
    assert _relerr(lpw.cpu().numpy(), lpf.cpu().numpy()) < 1e-6 and _relerr(gw.cpu().numpy(), gf.cpu().numpy()) < 1e-5
    _check(lpw, gw, *_ref(spec, prob, x=prob['x'][b:b + c], y=prob['y'][b:b + c]))
    small = R.synthetic_problem(spec, 3, 2, seed=5)           # fewer rows than row ranges: empty ranges write zeros
    eng.set_data(torch.from_numpy(small['X']), torch.from_numpy(small['y']))
    _check(*eng.logpost_grad(torch.from_numpy(small['theta0'])), *_ref(spec, {**small, 'emb': prob['emb'], 'pos': prob['pos']}))


def test_warmstart_steps_match_the_optax_rules():
    from mile_amd.warmstart import _Optimizer
    spec = _spec(80, 20, 40, 4, 16, 2, (8,), True)
    E, N, bs = 3, 64, 32
    prob = R.synthetic_problem(spec, N, E, seed=17)
    eng = _engine(spec, prob)
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
        lg = [R.loglik_and_grad(spec, t, prob['emb'], prob['pos'], prob['x'][r0:r0 + bs], prob['y'][r0:r0 + bs])
              for t in th_b.numpy().astype(np.float64)]
        nll_b = -np.array([ll for ll, _ in lg]) / bs
        gl = np.stack([g for _, g in lg])
        th_b = ref.step(th_b, torch.from_numpy((-gl / bs).astype(np.float32)), active)
        assert _relerr(nll_a[active.cuda()].cpu().numpy(), nll_b[active.numpy()]) < 1e-4, k
    eng.set_row_window(0, 0)
    torch.cuda.synchronize()
    assert torch.equal(th_a[1].cpu(), torch.from_numpy(prob['theta0'][1]))
    assert _relerr(th_a.cpu().numpy(), th_b.numpy()) < 5e-4
    assert _relerr(ost['m'].cpu().numpy(), ref.m.numpy()) < 1e-4 and _relerr(ost['v'].cpu().numpy(), ref.v.numpy()) < 1e-4


def test_pointwise_loglik_matches_restatement():
    spec = _spec(100, 30, 72, 4, 16, 3, (8,), True)
    prob = R.synthetic_problem(spec, 20, 5, seed=6)
    test = R.synthetic_problem(spec, 301, 1, seed=7)
    eng = _engine(spec, prob)
    pw = eng.pointwise_loglik(torch.from_numpy(prob['theta0']), torch.from_numpy(test['X']), torch.from_numpy(test['y']))
    ref = np.stack([R.pointwise_loglik(spec, t, prob['emb'], prob['pos'], test['x'], test['y']) for t in prob['theta0']])
    assert pw.shape == (5, 301)
    assert np.abs(pw.cpu().numpy() - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())


def test_mclmc_steps_match_oracle(oracle):
    spec = _spec(40, 12, 40, 4, 16, 2, (8,), False)
    N, E, T = 48, 3, 4
    prob = R.synthetic_problem(spec, N, E, seed=9)
    rng = np.random.default_rng(4)
    d = spec.n_params
    z0 = rng.standard_normal((E, d)).astype(np.float32)
    noise = rng.standard_normal((T, 2, E, d)).astype(np.float32)
    f = lambda th: _ref(spec, prob, theta=th)     # noqa: E731
    st = oracle.mclmc_init(f, prob['theta0'].astype(np.float64), z0.astype(np.float64))
    for i in range(T):
        st, info = oracle.mclmc_step(f, st, prob['eps'].astype(np.float64), prob['L'].astype(np.float64),
                                     noise[i, 0].astype(np.float64), noise[i, 1].astype(np.float64))
    eng = _engine(spec, prob)
    s = eng.init(torch.from_numpy(prob['theta0']), noise=torch.from_numpy(z0))
    s, info_g, _ = eng.step(s, torch.from_numpy(prob['eps']), torch.from_numpy(prob['L']), n_steps=T, noise=torch.from_numpy(noise))
    torch.cuda.synchronize()
    assert _relerr(s.position.cpu().numpy(), st.position) < 1e-4
    assert _relerr(s.logdensity.cpu().numpy(), st.logdensity) < 1e-5
    assert _relerr(s.logdensity_grad.cpu().numpy(), st.logdensity_grad) < 1e-3
    assert np.abs(info_g.energy_change[-1].cpu().numpy() - info.energy_change).max() < 5e-3


def test_nuts_step_teacher_forced():
    spec = _spec(30, 10, 24, 2, 8, 2, (8,), True)
    N, E, M, eps = 30, 3, 5, 0.01
    prob = R.synthetic_problem(spec, N, E, seed=12)
    d = spec.n_params
    rng = np.random.default_rng(12)
    z = rng.standard_normal((1, E, d)).astype(np.float32)
    u = rng.uniform(size=(1, E, 2 * M + 2 ** M)).astype(np.float32)
    m = rng.uniform(0.5, 1.5, (E, d)).astype(np.float32)

    def f(x):
        lp, g = _ref(spec, prob, theta=np.asarray(x, np.float64)[None])
        return float(lp[0]), g[0]

    eng = _engine(spec, prob)
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


def test_state_error_before_tables_and_new_tables_followed():
    """Every likelihood call fails with MILE_ERR_STATE until mile_set_embedding; new tables change the gradient to theirs."""
    import ctypes as C
    from mile_amd import _lib
    spec = _spec(60, 16, 32, 2, 16, 2, (8,), True)
    prob = R.synthetic_problem(spec, 20, 2, seed=8)
    lib = _lib.load_library()
    cs = _lib.ModelSpecC()
    cs.in_features, cs.n_layers = 16, 2
    cs.widths[0], cs.widths[1] = 8, 2
    cs.task, cs.prior, cs.prior_scale, cs.use_bias = 1, 0, 0.2, 1
    cs.model, cs.vocab_size, cs.ctx_len, cs.emb_size, cs.n_heads, cs.qkv_dim = 4, 60, 16, 32, 2, 16
    h = C.c_void_p()
    assert lib.mile_create(C.byref(cs), 0, C.byref(h)) == 0
    try:
        X, y = torch.from_numpy(prob['X']).cuda(), torch.from_numpy(prob['y']).cuda()
        th = torch.from_numpy(prob['theta0']).cuda()
        E, d = th.shape
        lp, g = torch.zeros(E, device='cuda'), torch.zeros(E, d, device='cuda')
        assert lib.mile_set_data(h, X.data_ptr(), y.data_ptr(), 20, None) == 0
        assert lib.mile_reserve(h, E) == 0
        assert lib.mile_logpost_grad(h, th.data_ptr(), E, lp.data_ptr(), g.data_ptr(), None) == -2
        assert b'mile_set_embedding' in lib.mile_last_error()
        out = torch.zeros(E, 20, device='cuda')
        assert lib.mile_pointwise_loglik(h, th.data_ptr(), E, X.data_ptr(), y.data_ptr(), 20, out.data_ptr(), None) == -2
        opt = _lib.OptimArgsC(kind=0, learning_rate=0.1, t=1)
        assert lib.mile_warmstart_step(h, th.data_ptr(), E, C.byref(opt), None) == -2
        u = torch.zeros_like(g)
        state = _lib.StateC(E, th.data_ptr(), u.data_ptr(), lp.data_ptr(), g.data_ptr())
        assert lib.mile_init(h, C.byref(state), None, 0, None, None) == -2
        eps, L = torch.full((E,), 1e-3, device='cuda'), torch.ones(E, device='cuda')
        step = _lib.StepArgsC(step_size=eps.data_ptr(), L=L.data_ptr(), n_steps=1)
        assert lib.mile_step(h, C.byref(state), C.byref(step), None) == -2
        assert lib.mile_nuts_reserve(h, E, 3) == 0
        nuts = _lib.NutsArgsC(step_size=eps.data_ptr(), inverse_mass_matrix=torch.ones(E, d, device='cuda').data_ptr(),
                              max_num_doublings=3, divergence_threshold=1000.0, n_steps=1)
        assert lib.mile_nuts_step(h, C.byref(state), C.byref(nuts), None) == -2
        torch.cuda.synchronize()
        assert float(g.abs().max()) == 0.0                   # nothing ran
    finally:
        lib.mile_destroy(h)
    eng = _engine(spec, prob)
    th = torch.from_numpy(prob['theta0'])
    _check(*eng.logpost_grad(th), *_ref(spec, prob))
    emb2, pos2 = R.tables(spec, seed=99, extra_pos_rows=3)
    eng.set_embedding(emb2, pos2)
    lp2, g2 = eng.logpost_grad(th)
    torch.cuda.synchronize()
    ref2 = _ref(spec, {**prob, 'emb': emb2, 'pos': pos2})
    _check(lp2, g2, *ref2)
    assert _relerr(ref2[1], _ref(spec, prob)[1]) > 1e-2       # the tables matter


def test_train_and_evaluate_cli(tmp_path):
    """tools/make_embeddings.py, then `train.py -c` on a shrunken copy of experiments/mclmc_seqmod_pretrained_synthetic.yaml,
    then `evaluate.py`.  Sample files hold the sampled leaves only."""
    import json
    import subprocess
    import sys
    from pathlib import Path

    import yaml
    root = Path(__file__).resolve().parents[1]
    tabs = tmp_path / 'tables' / 'emb_small.npy'
    r = subprocess.run([sys.executable, str(root / 'tools' / 'make_embeddings.py'), '--random', '50', '20', '40', '--seed', '1',
                        '--out', str(tabs)], capture_output=True, text=True, cwd=root, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / 'tables' / 'pos_emb_small.npy').exists()
    cfg = yaml.safe_load((root / 'experiments' / 'mclmc_seqmod_pretrained_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['experiment_name'] = 'seqpre_small'
    cfg['data']['path'] = '400x20x50'
    cfg['data']['datapoint_limit'] = 400
    cfg['model'].update(context_len=20, vocab_size=50, emb_size=40, emb_path=str(tabs))
    cfg['training']['warmstart'].update(max_epochs=2, patience=2)
    cfg['training']['sampler'].update(warmup_steps=30, n_samples=20, n_chains=3, n_thinning=10)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, str(root / 'train.py'), '-c', str(tmp_path / 'cfg.yaml'), '-d', '1'],
                       capture_output=True, text=True, cwd=root, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp = tmp_path / 'seqpre_small'
    assert 'Warmstart Training completed' in (exp / 'training.log').read_text()
    assert sorted(p.name for p in (exp / 'samples').iterdir() if p.is_dir()) == ['0', '1', '2']
    z = np.load(exp / 'samples' / '2' / 'sample_10.npz')
    assert z.files == ['MDPA.key.bias', 'MDPA.key.kernel', 'MDPA.out.bias', 'MDPA.out.kernel', 'MDPA.query.bias',
                       'MDPA.query.kernel', 'MDPA.value.bias', 'MDPA.value.kernel', 'classifier.bias', 'classifier.kernel',
                       'projection_0.bias', 'projection_0.kernel']
    assert z['MDPA.key.kernel'].shape == (40, 8, 8) and z['MDPA.out.kernel'].shape == (8, 8, 40)
    assert all(np.isfinite(z[k]).all() for k in z.files)
    r = subprocess.run([sys.executable, str(root / 'evaluate.py'), '-e', str(exp), '--split', 'valid'], capture_output=True,
                       text=True, cwd=root, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = json.loads((exp / 'metrics.json').read_text())
    assert m['split'] == 'valid' and m['n_points'] == 40 and np.isfinite(m['lppd'])
