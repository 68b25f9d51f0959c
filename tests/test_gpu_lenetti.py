"""LeNetti target on its HIP kernel (k_grad_lenetti / k_fwd_lenetti) vs the fp64 restatement tests/lenetti_ref.py (-m gpu)."""
import numpy as np
import pytest

from tests import leafcheck as L
from tests import lenetti_ref as R
from tests import nuts_ref as NR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


def _spec(ospec):
    from mile_amd import LeNettiSpec
    spec = LeNettiSpec(ospec.channels, ospec.height, ospec.width, ospec.out_dim, activation=ospec.activation, task=ospec.task,
                       prior=ospec.prior, prior_loc=ospec.prior_loc, prior_scale=ospec.prior_scale)
    assert spec.n_params == ospec.n_params
    assert [(n, o, tuple(s)) for n, o, s in spec.leaves()] == [(n, o, tuple(s)) for n, o, s in ospec.leaves()]
    return spec


def _engine(ospec, X, y, kernel='auto'):
    from mile_amd.engine import Engine
    eng = Engine(_spec(ospec), torch.from_numpy(X), torch.from_numpy(y), device='cuda:0', grad_kernel=kernel)
    assert eng.grad_kernel == 'lenetti_f32'
    return eng


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _check(lp, g, lp_ref, g_ref):
    """DESIGN section 1 tolerances: log-density 2e-5 relative, gradient 2e-5 of its largest entry (per chain)."""
    lp, g = lp.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    assert np.abs(lp - lp_ref).max() < 2e-5 * max(1.0, np.abs(lp_ref).max()), (lp, lp_ref)
    for e in range(g.shape[0]):
        assert np.abs(g[e] - g_ref[e]).max() < 2e-5 * np.abs(g_ref[e]).max(), e


CASES = [
    # C, H, W, out_dim, activation, task, prior, N, E
    (1, 28, 28, 10, 'relu', 'classification', 'Normal', 100, 3),     # MNIST-shaped (4 pixels per thread)
    (3, 32, 32, 10, 'sigmoid', 'classification', 'Normal', 37, 2),   # CIFAR-shaped (5 pixels per thread, tiles of 2)
    (2, 13, 17, 2, 'tanh', 'regr', 'Laplace', 29, 3),                # odd sizes, regression head
    (1, 1, 1, 3, 'relu', 'classification', 'Normal', 1, 1),          # smallest image, one row, one particle
    (4, 40, 40, 16, 'relu', 'classification', 'Normal', 11, 2),      # widest supported: 4 channels, 1764 pixels, 16 outputs
]


@pytest.mark.parametrize('C,H,W,K,act,task,prior,N,E', CASES)
def test_logpost_grad_matches_restatement(C, H, W, K, act, task, prior, N, E):
    ospec = R.LeNettiSpec(C, H, W, K, activation=act, task=task, prior=prior, prior_scale=0.7 if prior == 'Laplace' else 1.0)
    prob = R.synthetic_problem(ospec, N, E, seed=3)
    lp_ref, g_ref = R.logpost_and_grad(ospec, prob['theta0'].astype(np.float64), prob['X'], prob['y'])
    eng = _engine(ospec, prob['X'], prob['y'])
    lp, g = eng.logpost_grad(torch.from_numpy(prob['theta0']))
    torch.cuda.synchronize()
    _check(lp, g, lp_ref, g_ref)
    L.assert_leaves(g.cpu().numpy(), g_ref, L.spec_leaves(ospec), tag=(C, H, W, K, act))     # leaf by leaf: 5e-5 of the leaf's largest entry


def test_row_splits_and_windows():
    """E = 10 chains on 4 096 MNIST-shaped images; ensembles of 1, 10 and 40 chains split the rows into 64, 52 and 13 ranges.
    A row window gives what a fresh engine on those rows gives."""
    ospec = R.LeNettiSpec(1, 28, 28, 10, activation='relu')
    N = 4096
    prob = R.synthetic_problem(ospec, N, 10, seed=4)
    th64 = prob['theta0'].astype(np.float64)
    lp_ref, g_ref = R.logpost_and_grad(ospec, th64, prob['X'], prob['y'])
    eng = _engine(ospec, prob['X'], prob['y'])
    th = torch.from_numpy(prob['theta0'])
    _check(*eng.logpost_grad(th), lp_ref, g_ref)
    _check(*eng.logpost_grad(th[:1]), lp_ref[:1], g_ref[:1])
    lp40, g40 = eng.logpost_grad(th.repeat(4, 1))
    _check(lp40, g40, np.tile(lp_ref, 4), np.tile(g_ref, (4, 1)))
    b, c = 1000, 77
    eng.set_row_window(b, c)
    lpw, gw = eng.logpost_grad(th)
    eng.set_row_window(0, 0)
    fresh = _engine(ospec, np.ascontiguousarray(prob['X'][b:b + c]), np.ascontiguousarray(prob['y'][b:b + c]))
    lpf, gf = fresh.logpost_grad(th)
    assert _relerr(lpw.cpu().numpy(), lpf.cpu().numpy()) < 1e-6 and _relerr(gw.cpu().numpy(), gf.cpu().numpy()) < 1e-5
    lpr, gr = R.logpost_and_grad(ospec, th64, prob['X'][b:b + c], prob['y'][b:b + c])
    _check(lpw, gw, lpr, gr)


@pytest.mark.parametrize('C,H,W,K,task', [(1, 28, 28, 10, 'classification'), (3, 9, 11, 2, 'regr')])
def test_pointwise_loglik_matches_restatement(oracle, C, H, W, K, task):
    ospec = R.LeNettiSpec(C, H, W, K, activation='tanh', task=task)
    prob = R.synthetic_problem(ospec, 20, 5, seed=6)
    test = R.synthetic_problem(ospec, 301, 1, seed=7)
    eng = _engine(ospec, prob['X'], prob['y'])
    pw = eng.pointwise_loglik(torch.from_numpy(prob['theta0']), torch.from_numpy(test['X']), torch.from_numpy(test['y']))
    out = R.forward(ospec, prob['theta0'].astype(np.float64), test['X'])
    ref, _ = oracle.pointwise_loglik_raw(ospec, out, test['y'])
    assert pw.shape == (5, 301)
    assert np.abs(pw.cpu().numpy() - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())


def test_mclmc_steps_match_oracle(oracle):
    ospec = R.LeNettiSpec(1, 12, 12, 4, activation='sigmoid')
    N, E, T = 64, 3, 4
    prob = R.synthetic_problem(ospec, N, E, seed=9)
    rng = np.random.default_rng(4)
    d = ospec.n_params
    z0 = rng.standard_normal((E, d)).astype(np.float32)
    noise = rng.standard_normal((T, 2, E, d)).astype(np.float32)
    f = lambda th: R.logpost_and_grad(ospec, th, prob['X'], prob['y'])
    st = oracle.mclmc_init(f, prob['theta0'].astype(np.float64), z0.astype(np.float64))
    for i in range(T):
        st, info = oracle.mclmc_step(f, st, prob['eps'].astype(np.float64), prob['L'].astype(np.float64),
                                     noise[i, 0].astype(np.float64), noise[i, 1].astype(np.float64))
    eng = _engine(ospec, prob['X'], prob['y'])
    s = eng.init(torch.from_numpy(prob['theta0']), noise=torch.from_numpy(z0))
    s, info_g, _ = eng.step(s, torch.from_numpy(prob['eps']), torch.from_numpy(prob['L']), n_steps=T, noise=torch.from_numpy(noise))
    torch.cuda.synchronize()
    assert _relerr(s.position.cpu().numpy(), st.position) < 1e-4
    assert _relerr(s.logdensity.cpu().numpy(), st.logdensity) < 1e-5
    assert _relerr(s.logdensity_grad.cpu().numpy(), st.logdensity_grad) < 1e-3
    assert np.abs(info_g.energy_change[-1].cpu().numpy() - info.energy_change).max() < 5e-3


def test_nuts_step_teacher_forced():
    ospec = R.LeNettiSpec(1, 10, 10, 3, activation='tanh')
    N, E, M, eps = 50, 3, 5, 0.01
    prob = R.synthetic_problem(ospec, N, E, seed=12)
    d = ospec.n_params
    rng = np.random.default_rng(12)
    z = rng.standard_normal((1, E, d)).astype(np.float32)
    u = rng.uniform(size=(1, E, 2 * M + 2 ** M)).astype(np.float32)
    m = rng.uniform(0.5, 1.5, (E, d)).astype(np.float32)

    def f(x):
        lp, g = R.logpost_and_grad(ospec, np.asarray(x, np.float64)[None], prob['X'], prob['y'])
        return float(lp[0]), g[0]

    eng = _engine(ospec, prob['X'], prob['y'])
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


def test_full_size_permutation_and_finiteness():
    """E = 128 chains on 48 000 MNIST-shaped images (the reference run's training rows): permuting the particles permutes the
    outputs bit for bit, nothing is NaN, and a few MCLMC steps stay finite with unit momenta."""
    from mile_amd import LeNettiSpec
    from mile_amd.engine import Engine
    N, E = 48000, 128
    rng = np.random.default_rng(0)
    X = torch.from_numpy(rng.standard_normal((N, 1, 28, 28)).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, 10, N).astype(np.int32))
    spec = LeNettiSpec(1, 28, 28, 10, activation='relu')
    eng = Engine(spec, X, y, device='cuda:0')
    th = torch.from_numpy((0.03 * rng.standard_normal((E, spec.n_params))).astype(np.float32))
    lp, g = eng.logpost_grad(th)
    assert torch.isfinite(lp).all() and torch.isfinite(g).all()
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(1))
    lp2, g2 = eng.logpost_grad(th[perm])
    assert torch.equal(lp2.cpu(), lp.cpu()[perm]) and torch.equal(g2.cpu(), g.cpu()[perm])
    ids = torch.arange(E, dtype=torch.int32)
    s0 = eng.init(th, seed=5, particle_ids=ids)
    s1, info, _ = eng.step(s0, torch.full((E,), 1e-3), torch.full((E,), 1.0), n_steps=3, seed=5, particle_ids=ids)
    assert torch.isfinite(s1.position).all() and torch.isfinite(info.energy_change).all()
    assert (s1.momentum.double().norm(dim=1) - 1).abs().max().item() < 1e-5


def test_train_and_evaluate_cli(tmp_path):
    """`train.py -c` on a shrunken copy of experiments/mclmc_lenetti_mnist.yaml (warm start on row windows, 30 + 20 MCLMC
    steps), then `evaluate.py`."""
    import json
    import subprocess
    import sys
    from pathlib import Path

    import yaml
    root = Path(__file__).resolve().parents[1]
    cfg = yaml.safe_load((root / 'experiments' / 'mclmc_lenetti_mnist.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['experiment_name'] = 'lenetti_small'
    cfg['data']['path'] = '400x1x12x12'
    cfg['data']['datapoint_limit'] = 400
    cfg['training']['warmstart'].update(max_epochs=3, patience=2)
    cfg['training']['sampler'].update(warmup_steps=30, n_samples=20, n_chains=3, n_thinning=10)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, str(root / 'train.py'), '-c', str(tmp_path / 'cfg.yaml'), '-d', '1'],
                       capture_output=True, text=True, cwd=root, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp = tmp_path / 'lenetti_small'
    assert 'Warmstart Training completed' in (exp / 'training.log').read_text()
    assert sorted(p.name for p in (exp / 'samples').iterdir() if p.is_dir()) == ['0', '1', '2']
    z = np.load(exp / 'samples' / '2' / 'sample_10.npz')
    assert z.files == ['core.conv1.bias', 'core.conv1.kernel', 'core.fc1.bias', 'core.fc1.kernel', 'core.fc2.bias',
                       'core.fc2.kernel', 'core.fc3.bias', 'core.fc3.kernel', 'core.fc4.bias', 'core.fc4.kernel']
    assert z['core.conv1.kernel'].shape == (3, 3, 1, 1) and z['core.fc1.kernel'].shape == (14 * 14, 8)
    assert all(np.isfinite(z[k]).all() for k in z.files)
    r = subprocess.run([sys.executable, str(root / 'evaluate.py'), '-e', str(exp), '--split', 'valid'], capture_output=True,
                       text=True, cwd=root, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = json.loads((exp / 'metrics.json').read_text())
    assert m['split'] == 'valid' and m['n_points'] == 40 and np.isfinite(m['lppd'])
