"""AttentionClassifier at emb_size <= 192 on its HIP kernel (k_grad_attn_wide / k_fwd_attn_wide) vs the fp64 restatement
tests/attn_ref.py (-m gpu).  Tolerances are the project's own (tests/test_gpu_attn*.py, tests/leafcheck.py)."""
import numpy as np
import pytest

from tests import attn_ref as R
from tests import leafcheck as L
from tests import nuts_ref as NR
from tests.test_attn_wide_host import LEAF_CASES, leaf_problem, wide_spec

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


def _engine(spec, prob, X=None, y=None):
    from mile_amd.engine import Engine
    X = prob['X'] if X is None else X
    y = prob['y'] if y is None else y
    eng = Engine(spec, torch.from_numpy(np.ascontiguousarray(X)), torch.from_numpy(np.ascontiguousarray(y)), device='cuda:0')
    assert eng.grad_kernel == 'attn_wide_f32'
    return eng


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _ref(spec, prob, theta=None, x=None, y=None):
    return R.logpost_and_grad(spec, prob['theta0'] if theta is None else theta, prob['x'] if x is None else x,
                              prob['y'] if y is None else y)


def _check(lp, g, lp_ref, g_ref):
    """DESIGN section 1 tolerances: log-density 2e-5 relative, gradient 2e-5 of its largest entry (per chain)."""
    lp, g = lp.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    print('LOGP relerr %.2e' % (np.abs(lp - lp_ref).max() / max(1.0, np.abs(lp_ref).max())))
    assert np.abs(lp - lp_ref).max() < 2e-5 * max(1.0, np.abs(lp_ref).max()), (lp, lp_ref)
    for e in range(g.shape[0]):
        err = np.abs(g[e] - g_ref[e])
        print('GRAD chain %d relerr %.2e' % (e, err.max() / np.abs(g_ref[e]).max()))
        assert err.max() < 2e-5 * np.abs(g_ref[e]).max(), (e, int(err.argmax()), err.max(), np.abs(g_ref[e]).max())


CASES = [
    # V, T, C, H, D, K, proj, bias, N, E
    (10000, 70, 192, 8, 64, 2, (32,), True, 24, 2),          # sequential_mod_pretraining.yaml (hd = 8), d = 1 989 218
    (10000, 70, 192, 10, 100, 2, (128, 32), True, 20, 1),    # sequential_mod_pretraining_larger.yaml (hd = 10), d = 2 039 630
    (300, 37, 61, 2, 32, 3, (20,), False, 17, 2),            # C, T not multiples of 16, hd = 16, K = 3, no bias
    (200, 50, 100, 2, 64, 2, (), True, 9, 3),                # hd = 32 (dK in LDS), no projection
    (50, 16, 24, 1, 100, 2, (128, 8), False, 5, 1),          # one head of 100 (seven dq tiles), two projections
    (80, 128, 64, 4, 64, 16, (16,), True, 4, 2),             # T = 128, K = 16
    (1000, 70, 48, 8, 64, 2, (32,), True, 24, 2),            # inside k_grad_attn's envelope, forced onto the wide kernel
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
    spec = wide_spec(V, T, C, H, D, K, proj, bias)
    prob = R.synthetic_problem(spec, N, E, seed=3)
    eng = _engine(spec, prob)
    lp, g = eng.logpost_grad(torch.from_numpy(prob['theta0']))
    torch.cuda.synchronize()
    _check(lp, g, *_ref(spec, prob))
    info = eng.grad_launch_info(E)
    assert info['lds_bytes'] == spec.lds_bytes and info['kernel'] == 'k_grad_attn_wide'
    if C <= 64 and D <= 64 and all(p <= 64 for p in proj):   # the same problem on the on-chip kernel
        from mile_amd.engine import Engine
        from mile_amd.spec import AttentionSpec
        small = AttentionSpec(V, T, C, H, D, n_classes=K, projection_dim=proj, use_bias=bias, prior='Normal', prior_scale=0.2)
        e2 = Engine(small, torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device='cuda:0')
        assert e2.grad_kernel == 'attn_f32'
        lp2, g2 = e2.logpost_grad(torch.from_numpy(prob['theta0']))
        torch.cuda.synchronize()
        assert _relerr(lp.cpu().numpy(), lp2.cpu().numpy()) < 2e-5 and _relerr(g.cpu().numpy(), g2.cpu().numpy()) < 4e-5


@pytest.mark.parametrize('case', LEAF_CASES)
def test_gradient_per_leaf(case):
    """Every leaf of every chain against fp64 on the sharp problem under prior_scale 1000 (tests/test_attn_wide_host.py asserts
    that every leaf's gradient is the likelihood's there): 5e-5 of the leaf's own maximum or 8x the float32 restatement's own
    error (leafcheck.leaf_bounds); MDPA.key.bias on the query bias's scale.  The embedding table is the leaf that would hide a
    dropped duplicate-token add."""
    P = leaf_problem(*case)
    eng = _engine(P.spec, P.prob)
    lp, g = eng.logpost_grad(torch.from_numpy(P.prob['theta0']))
    torch.cuda.synchronize()
    lp_ref, g_ref = P.ref()
    _, g32 = P.ref(np.float32)
    bound = P.bound(g_ref)
    g = g.cpu().numpy().astype(np.float64)
    err, err32 = L.leaf_errors(g, g_ref, P.leaves, P.scale_of), L.leaf_errors(g32, g_ref, P.leaves, P.scale_of)
    print(f'\nLEAFPARITY wide {case}')
    for j, (n, _, _) in enumerate(P.leaves):
        print(f'LEAF {n:<48s} device {err[:, j].max():.2e}  float32 restatement {err32[:, j].max():.2e}  bound {bound[:, j].min():.2e}')
    lp = lp.cpu().numpy().astype(np.float64)
    assert np.abs(lp - lp_ref).max() < 2e-5 * max(1.0, np.abs(lp_ref).max()), (lp, lp_ref)
    L.assert_leaves(g, g_ref, P.leaves, bound, P.scale_of, tag=('wide',) + tuple(case))


def test_row_splits_and_windows():
    """Ensembles of 1, 2 and 4 chains split the rows into different ranges; a row window gives what a fresh engine on those rows
    gives and what the restatement gives on them; two gradients in a row on different windows, the second touching fewer tokens
    (a stale table block would show); fewer rows than row ranges writes zeros, the table block included."""
    spec = wide_spec(300, 24, 72, 4, 32, 2, (16,), True)
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
    fresh = _engine(spec, prob, prob['X'][b:b + c], prob['y'][b:b + c])
    lpf, gf = fresh.logpost_grad(th)
    assert _relerr(lpw.cpu().numpy(), lpf.cpu().numpy()) < 1e-6 and _relerr(gw.cpu().numpy(), gf.cpu().numpy()) < 1e-5
    _check(lpw, gw, *_ref(spec, prob, x=prob['x'][b:b + c], y=prob['y'][b:b + c]))
    b2, c2 = 300, 9                                             # straight after: fewer rows, fewer distinct tokens
    assert len(np.unique(prob['x'][b2:b2 + c2])) < len(np.unique(prob['x'][b:b + c]))
    eng.set_row_window(b2, c2)
    lp2, g2 = eng.logpost_grad(th)
    eng.set_row_window(0, 0)
    _check(lp2, g2, *_ref(spec, prob, x=prob['x'][b2:b2 + c2], y=prob['y'][b2:b2 + c2]))
    emb = [(o, int(np.prod(s))) for n, o, s in spec.leaves() if n.endswith('Embedding.embedding') and 'Position' not in n][0]
    untouched = np.setdiff1d(np.arange(spec.vocab_size), prob['x'][b2:b2 + c2])
    blk = g2.cpu().numpy()[:, emb[0]:emb[0] + emb[1]].reshape(2, spec.vocab_size, spec.emb_size)
    pri = -prob['theta0'][:, emb[0]:emb[0] + emb[1]].reshape(blk.shape) / np.float32(0.2) ** 2
    assert np.abs(blk[:, untouched] - pri[:, untouched]).max() <= 1e-6 * np.abs(pri).max()   # the prior's gradient alone
    small = R.synthetic_problem(spec, 3, 2, seed=5)            # fewer rows than row ranges
    eng.set_data(torch.from_numpy(small['X']), torch.from_numpy(small['y']))
    _check(*eng.logpost_grad(torch.from_numpy(small['theta0'])), *_ref(spec, small))


@pytest.mark.parametrize('E', [1, 8])
def test_reserved_slabs_are_what_the_spec_reports(E):
    """mile_reserve at the stock shape on N = 35 000 rows: the bytes the library holds (mile_slab_bytes) are
    WideAttentionSpec.slab_bytes -- 256 slab rows, 2.04 GB, for one chain and for eight -- and the launch has that many ranges."""
    spec = wide_spec(10000, 70, 192, 8, 64, 2, (32,), True)
    N = 35000
    rng = np.random.default_rng(0)
    X = rng.integers(1, 10000, (N, 70)).astype(np.float32)
    y = rng.integers(0, 2, N).astype(np.int32)
    eng = _engine(spec, None, X, y)
    assert eng.slab_bytes == 0
    eng.reserve(E)
    assert eng.grad_launch_info(E)['grid'][0] == spec.row_splits(E, N) == 256 // E
    print('SLAB E %d library %d spec %d' % (E, eng.slab_bytes, spec.slab_bytes(E, N)))
    assert eng.slab_bytes == spec.slab_bytes(E, N) == 256 * 1_989_220 * 4
    eng.set_row_window(0, 256)                                  # a minibatch: fewer ranges, and nothing is reallocated
    eng.reserve(E)
    assert eng.grad_launch_info(E)['grid'][0] == spec.row_splits(E, 256) and eng.slab_bytes == spec.slab_bytes(E, N)


def test_full_shape_on_all_row_ranges(oracle):
    """d = 1 989 218 with S = 256 row ranges (2.04 GB of slabs: offsets beyond 32 bits in the grad kernel, k_finalize and the
    segmented update).  The data are 24 rows repeated 86 times, so the fp64 reference is 86 x the 24-row likelihood (and its
    gradient) plus the prior: the restatement stays at half a second.
    Position, log-density and gradient are held to the bounds of test_mclmc_steps_match_oracle.  The energy change is
    dK - (logp_new - logp_old) with both log-densities held in fp32 by the ABI; here |logp| = 1.37e6 (the prior's constant,
    -d (log 0.2 + 0.919)), where one fp32 step is 0.125, and unlike the 24-row case the log-density really moves between the two
    (86 x the likelihood gradient).  Each of the two stored values is within half a step of its own fp32 sum, whose inputs carry
    the log-density's 1e-5 relative allowance no further than that; the bound is therefore two fp32 steps at |logp| (0.25),
    never less than the 5e-3 used elsewhere."""
    from oracle import mclmc_oracle as M
    spec = wide_spec(10000, 70, 192, 8, 64, 2, (32,), True)
    reps = 86
    prob = R.synthetic_problem(spec, 24, 1, seed=3)
    X, y = np.tile(prob['X'], (reps, 1)), np.tile(prob['y'], reps)
    eng = _engine(spec, prob, X, y)
    assert eng.grad_launch_info(1)['grid'][0] == 256

    def f(th):
        th = np.asarray(th, np.float64)
        lls, gs = zip(*(R.loglik_and_grad(spec, t, prob['x'], prob['y']) for t in th))
        lp, gp = M.log_prior(spec, th)
        return reps * np.asarray(lls) + lp, reps * np.stack(gs) + gp

    lp, g = eng.logpost_grad(torch.from_numpy(prob['theta0']))
    torch.cuda.synchronize()
    _check(lp, g, *f(prob['theta0']))
    rng = np.random.default_rng(4)
    d = spec.n_params
    z0 = rng.standard_normal((1, d)).astype(np.float32)
    noise = rng.standard_normal((1, 2, 1, d)).astype(np.float32)
    st = oracle.mclmc_init(f, prob['theta0'].astype(np.float64), z0.astype(np.float64))
    st, info = oracle.mclmc_step(f, st, prob['eps'].astype(np.float64), prob['L'].astype(np.float64), noise[0, 0].astype(np.float64),
                                 noise[0, 1].astype(np.float64))
    s = eng.init(torch.from_numpy(prob['theta0']), noise=torch.from_numpy(z0))
    s, info_g, _ = eng.step(s, torch.from_numpy(prob['eps']), torch.from_numpy(prob['L']), n_steps=1, noise=torch.from_numpy(noise))
    torch.cuda.synchronize()
    print('MCLMC S=256 pos %.2e logp %.2e grad %.2e dE %.2e' % (
        _relerr(s.position.cpu().numpy(), st.position), _relerr(s.logdensity.cpu().numpy(), st.logdensity),
        _relerr(s.logdensity_grad.cpu().numpy(), st.logdensity_grad),
        np.abs(info_g.energy_change[-1].cpu().numpy() - info.energy_change).max()))
    assert _relerr(s.position.cpu().numpy(), st.position) < 1e-4
    assert _relerr(s.logdensity.cpu().numpy(), st.logdensity) < 1e-5
    assert _relerr(s.logdensity_grad.cpu().numpy(), st.logdensity_grad) < 1e-3
    e_bound = max(5e-3, 2.0 * float(np.spacing(np.float32(np.abs(st.logdensity).max()))))
    print('energy bound %.3g' % e_bound)
    assert np.abs(info_g.energy_change[-1].cpu().numpy() - info.energy_change).max() < e_bound


def test_warmstart_steps_match_the_optax_rules():
    from mile_amd.warmstart import _Optimizer
    spec = wide_spec(80, 20, 72, 4, 16, 2, (8,), True)
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
        lg = [R.loglik_and_grad(spec, t, prob['x'][r0:r0 + bs], prob['y'][r0:r0 + bs]) for t in th_b.numpy().astype(np.float64)]
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
    spec = wide_spec(100, 30, 72, 4, 16, 3, (8,), True)
    prob = R.synthetic_problem(spec, 20, 5, seed=6)
    test = R.synthetic_problem(spec, 301, 1, seed=7)
    eng = _engine(spec, prob)
    pw = eng.pointwise_loglik(torch.from_numpy(prob['theta0']), torch.from_numpy(test['X']), torch.from_numpy(test['y']))
    ref = np.stack([R.pointwise_loglik(spec, t, test['x'], test['y']) for t in prob['theta0']])
    assert pw.shape == (5, 301)
    assert np.abs(pw.cpu().numpy() - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize('shape,N,E,T', [((40, 12, 72, 4, 16, 2, (8,), False), 48, 3, 4),
                                         ((10000, 70, 192, 8, 64, 2, (32,), True), 24, 1, 2)], ids=['small', 'stock-d-1989218'])
def test_mclmc_steps_match_oracle(oracle, shape, N, E, T):
    """The second case is the reference's stock shape: what exercises the segmented update, k_finalize and the record path at
    d = 1 989 218."""
    spec = wide_spec(*shape)
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
    print('MCLMC pos %.2e logp %.2e grad %.2e dE %.2e' % (
        _relerr(s.position.cpu().numpy(), st.position), _relerr(s.logdensity.cpu().numpy(), st.logdensity),
        _relerr(s.logdensity_grad.cpu().numpy(), st.logdensity_grad),
        np.abs(info_g.energy_change[-1].cpu().numpy() - info.energy_change).max()))
    assert _relerr(s.position.cpu().numpy(), st.position) < 1e-4
    assert _relerr(s.logdensity.cpu().numpy(), st.logdensity) < 1e-5
    assert _relerr(s.logdensity_grad.cpu().numpy(), st.logdensity_grad) < 1e-3
    assert np.abs(info_g.energy_change[-1].cpu().numpy() - info.energy_change).max() < 5e-3


def test_nuts_step_teacher_forced():
    spec = wide_spec(30, 10, 72, 2, 8, 2, (8,), True)
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


def test_pretraining_pipeline_cli(tmp_path):
    """The three commands of the README on shrunk experiments: train.py on the pretraining YAML (emb_size 192), then
    tools/make_embeddings.py --from the warm start's parameters, then train.py on the pretrained YAML whose emb_path is that
    file, then evaluate.py.  The extracted tables are the warm start's leaves bit for bit."""
    import json
    import subprocess
    import sys
    from pathlib import Path

    import yaml
    root = Path(__file__).resolve().parents[1]
    V, T = 200, 24

    def run(*args):
        r = subprocess.run([sys.executable] + [str(a) for a in args], capture_output=True, text=True, cwd=root, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return r

    def shrink(name, exp, **model):
        cfg = yaml.safe_load((root / 'experiments' / name).read_text())
        cfg['saving_dir'] = str(tmp_path)
        cfg['experiment_name'] = exp
        cfg['data']['path'] = f'400x{T}x{V}'
        cfg['data']['datapoint_limit'] = 400
        cfg['model'].update(context_len=T, vocab_size=V, **model)
        cfg['training']['warmstart'].update(max_epochs=2, patience=2, batch_size=64)
        cfg['training']['sampler'].update(warmup_steps=20, n_samples=10, n_thinning=5)
        (tmp_path / f'{exp}.yaml').write_text(yaml.safe_dump(cfg))
        return tmp_path / f'{exp}.yaml'

    run(root / 'train.py', '-c', shrink('mclmc_seqmod_pretraining_synthetic.yaml', 'pre_training'), '-d', '1')
    exp1 = tmp_path / 'pre_training'
    assert 'Warmstart Training completed' in (exp1 / 'training.log').read_text()
    z = np.load(exp1 / 'warmstart' / 'params_0.npz')
    assert z['TokenEmbedding_0.Embedding.embedding'].shape == (V, 192)
    s = np.load(exp1 / 'samples' / '0' / 'sample_5.npz')
    assert s['TokenEmbedding_0.Embedding.embedding'].shape[-2:] == (V, 192) and all(np.isfinite(s[k]).all() for k in s.files)
    tabs = tmp_path / 'tables' / 'emb.npy'
    run(root / 'tools' / 'make_embeddings.py', '--from', exp1 / 'warmstart' / 'params_0.npz', '--out', tabs)
    assert np.array_equal(np.load(tabs), z['TokenEmbedding_0.Embedding.embedding'])
    assert np.array_equal(np.load(tmp_path / 'tables' / 'pos_emb.npy'), z['TokenEmbedding_0.PositionEmbedding.embedding'])
    cfg2 = shrink('mclmc_seqmod_pretrained_synthetic.yaml', 'pre_trained', emb_path=str(tabs))
    raw = yaml.safe_load(cfg2.read_text())
    raw['training']['sampler']['n_chains'] = 2
    cfg2.write_text(yaml.safe_dump(raw))
    run(root / 'train.py', '-c', cfg2, '-d', '1')
    exp2 = tmp_path / 'pre_trained'
    run(root / 'evaluate.py', '-e', exp2, '--split', 'valid')
    m = json.loads((exp2 / 'metrics.json').read_text())
    assert m['split'] == 'valid' and m['n_points'] == 40 and np.isfinite(m['lppd'])
    run(root / 'evaluate.py', '-e', exp1, '--split', 'valid')
    assert np.isfinite(json.loads((exp1 / 'metrics.json').read_text())['lppd'])
