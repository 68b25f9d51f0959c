"""mile_nuts_step / mile_nuts_warmup against the fp64 restatement (tests/nuts_ref.py), explicit draws (-m gpu)."""
import json
import pickle
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import nuts_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
ROOT = Path(__file__).resolve().parents[1]


def _engine(oracle, ospec, prob, kernel='auto'):
    from mile_amd import ModelSpec
    from mile_amd.engine import Engine
    spec = ModelSpec(in_features=ospec.in_features, hidden_structure=ospec.hidden_structure,
                     activation=ospec.activation, task=ospec.task, prior=ospec.prior,
                     prior_loc=ospec.prior_loc, prior_scale=ospec.prior_scale)
    return Engine(spec, torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device='cuda:0', grad_kernel=kernel)


def _f(oracle, ospec, prob):
    def f(x):
        lp, g = oracle.logpost_and_grad(ospec, np.asarray(x, np.float64)[None], prob['X'], prob['y'])
        return float(lp[0]), g[0]
    return f


def _draws(rng, T, E, d, M):
    return (rng.standard_normal((T, E, d)).astype(np.float32),
            rng.uniform(size=(T, E, 2 * M + 2 ** M)).astype(np.float32))


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _teacher_forced(oracle, ospec, kernel, N, E, T, eps, M, seed, m_scale=1.0):
    """Every step starts from the restatement's state; the device's step from there is compared with the
    restatement's.  Returns the per-step info arrays of both."""
    prob = oracle.synthetic_problem(ospec, N, E, seed=seed)
    d = ospec.n_params
    rng = np.random.default_rng(seed)
    z, u = _draws(rng, T, E, d, M)
    m = (m_scale * rng.uniform(0.5, 1.5, (E, d))).astype(np.float32)
    f = _f(oracle, ospec, prob)
    eng = _engine(oracle, ospec, prob, kernel)
    if kernel != 'auto':
        assert eng.grad_kernel == kernel
    x = prob['theta0'].astype(np.float32)
    n_div = n_exp = 0
    for i in range(T):
        s0 = eng.nuts_init(torch.from_numpy(x))
        s1, info, _ = eng.nuts_step(s0, torch.full((E,), eps), torch.from_numpy(m), max_num_doublings=M,
                                    noise=torch.from_numpy(z[i:i + 1]), uniforms=torch.from_numpy(u[i:i + 1]))
        torch.cuda.synchronize()
        got = np.stack([t[0].cpu().numpy() for t in info], axis=1)         # [E, 6]
        xr = np.empty_like(x)
        for e in range(E):
            lp, g = f(x[e])
            st, inf = R.nuts_step(f, R.HMCState(x[e].astype(np.float64), lp, g), float(np.float32(eps)),
                                  m[e].astype(np.float64), z[i, e].astype(np.float64), u[i, e].astype(np.float64), M)
            want = (inf.num_integration_steps, inf.num_trajectory_expansions, inf.is_divergent, inf.is_turning)
            assert tuple(int(v) for v in got[e, [0, 2, 3, 5]]) == tuple(int(v) for v in want), (i, e, got[e], inf)
            assert abs(got[e, 1] - inf.acceptance_rate) < 1e-3 + 1e-3 * inf.acceptance_rate, (i, e)
            assert abs(got[e, 4] - inf.energy) < 2e-3 * max(1.0, abs(inf.energy)), (i, e)
            assert _relerr(s1.position[e].cpu().numpy(), st.position) < 1e-3, (i, e)
            assert abs(float(s1.logdensity[e]) - st.logdensity) < 2e-4 * max(1.0, abs(st.logdensity)), (i, e)
            xr[e] = st.position
            n_div += inf.is_divergent
            n_exp += inf.num_trajectory_expansions
        x = xr.astype(np.float32)
    return n_div, n_exp / (T * E)


@pytest.mark.parametrize('hs,task,prior,kernel', [
    ((16, 16, 2), 'regr', 'Normal', 'mfma_narrow_f32'),
    ((16, 16, 3), 'classification', 'Laplace', 'mfma_narrow_f32'),
    ((64, 64, 64, 2), 'regr', 'Normal', 'mfma_w64'),
    ((16, 16, 2), 'regr', 'Laplace', 'generic'),
])
def test_teacher_forced_steps_match_the_restatement(oracle, hs, task, prior, kernel):
    ospec = oracle.ModelSpec(5, hs, task=task, prior=prior)
    _, mean_exp = _teacher_forced(oracle, ospec, kernel, N=200, E=4, T=20, eps=0.02 if len(hs) == 3 else 0.005, M=6,
                                  seed=7)
    assert mean_exp > 1.5        # the trees had depth: U-turn checkpoints and biased sampling were exercised


def test_teacher_forced_steps_at_large_d(oracle):
    """d = 17 538: every per-chain reduction runs over many strides of the workgroup."""
    ospec = oracle.ModelSpec(5, (128, 128, 2))
    assert ospec.n_params > 16384
    _teacher_forced(oracle, ospec, 'generic', N=100, E=2, T=3, eps=0.002, M=4, seed=3)


def test_first_leaf_divergence_leaves_the_state_unchanged(oracle):
    ospec = oracle.ModelSpec(5, (16, 16, 2))
    prob = oracle.synthetic_problem(ospec, 200, 3, seed=2)
    eng = _engine(oracle, ospec, prob)
    s0 = eng.nuts_init(torch.from_numpy(prob['theta0']))
    s1, info, _ = eng.nuts_step(s0, 50.0, 1.0, n_steps=1, seed=9)
    torch.cuda.synchronize()
    assert (info.is_divergent[0] == 1).all() and (info.num_trajectory_expansions[0] == 1).all()
    assert (info.num_integration_steps[0] == 1).all()
    assert torch.equal(s1.position, s0.position) and torch.equal(s1.logdensity, s0.logdensity)


def test_tiny_step_size_runs_to_max_num_doublings(oracle):
    ospec = oracle.ModelSpec(5, (16, 16, 2))
    prob = oracle.synthetic_problem(ospec, 200, 3, seed=2)
    eng = _engine(oracle, ospec, prob)
    s0 = eng.nuts_init(torch.from_numpy(prob['theta0']))
    stats = (__import__('ctypes').c_int64 * 2)(0, 0)
    M = 7
    s1, info, _ = eng.nuts_step(s0, 1e-7, 1.0, n_steps=2, max_num_doublings=M, seed=9, stats=stats)
    torch.cuda.synchronize()
    assert (info.num_integration_steps == 2 ** M - 1).all() and (info.num_trajectory_expansions == M).all()
    assert (info.is_divergent == 0).all() and (info.is_turning == 0).all()
    assert tuple(stats) == (2 * (2 ** M - 1), 2 * (M - 1))     # rounds launched; one host sync per doubling but the last


@pytest.mark.parametrize('T', [100, 300])
def test_window_adaptation_teacher_forced(oracle, T):
    """Each warm-up step starts from the restatement's chain AND adaptation state; step size, dual-averaging state and
    inverse mass matrix after the step are compared."""
    from mile_amd.warmup import build_schedule
    ospec = oracle.ModelSpec(5, (16, 16, 2))
    E, M = 2, 5
    prob = oracle.synthetic_problem(ospec, 150, E, seed=4)
    d = ospec.n_params
    rng = np.random.default_rng(T)
    z, u = _draws(rng, T, E, d, M)
    f = _f(oracle, ospec, prob)
    eng = _engine(oracle, ospec, prob)
    sched = build_schedule(T)
    ads = [R.WindowAdaptation(d, initial_step_size=0.05) for _ in range(E)]
    ad = eng.nuts_adaptation_init(E, 0.05)
    x = prob['theta0'].astype(np.float64)
    window_ends = flips = 0
    for i in range(T):
        for e, a in enumerate(ads):   # the restatement's adaptation state -> the device's
            ad['step_size'][e] = a.step_size
            ad['inverse_mass_matrix'][e] = torch.from_numpy(a.imm.astype(np.float32))
            ad['da'][e] = torch.tensor([a.da.log_x, a.da.log_x_avg, a.da.step, a.da.avg_grad, a.da.mu])
            ad['welford'][e, 0] = torch.from_numpy(a.mean.astype(np.float32))
            ad['welford'][e, 1] = torch.from_numpy(a.m2.astype(np.float32))
            ad['welford_count'][e] = a.n
        s = eng.nuts_init(torch.from_numpy(x.astype(np.float32)))
        info, _ = eng.nuts_warmup(s, ad, sched[i:i + 1], max_num_doublings=M, noise=torch.from_numpy(z[i:i + 1]),
                                  uniforms=torch.from_numpy(u[i:i + 1]), want_info=True)
        torch.cuda.synchronize()
        for e, a in enumerate(ads):
            lp, g = f(x[e])
            st, inf = R.nuts_step(f, R.HMCState(x[e], lp, g), float(np.float32(a.step_size)), a.imm.astype(np.float32),
                                  z[i, e].astype(np.float64), u[i, e].astype(np.float64), M)
            # the adaptation is teacher-forced too: it sees the device's acceptance rate and position.  Once dual averaging
            # has pushed eps to the edge of stability, fp32 rounding inside a 31-leaf trajectory moves the acceptance rate
            # by a few percent (same tree); the step itself is pinned by test_teacher_forced_steps_match_the_restatement.
            acc_dev, x_dev = float(info.acceptance_rate[0, e]), s.position[e].cpu().numpy().astype(np.float64)
            a.update(sched[i][0], sched[i][1], x_dev, acc_dev)
            x[e] = st.position
            if (int(info.num_integration_steps[0, e]), int(info.is_turning[0, e])) != (inf.num_integration_steps,
                                                                                      int(inf.is_turning)):
                flips += 1     # a U-turn dot product within fp32 rounding of zero: different trees
            else:
                assert abs(acc_dev - inf.acceptance_rate) < 0.1, (i, e)
            assert abs(float(ad['step_size'][e]) - a.step_size) < 1e-4 * a.step_size, (i, e)
            assert abs(float(ad['da'][e, 1]) - a.da.log_x_avg) < 2e-3 * max(1.0, abs(a.da.log_x_avg)), (i, e)
            if sched[i][1]:
                window_ends += 1
                assert _relerr(ad['inverse_mass_matrix'][e].cpu().numpy(), a.imm) < 1e-4, (i, e)
                assert float(ad['welford_count'][e]) == 0 and float(ad['da'][e, 2]) == 1
    assert flips <= max(1, T * E // 100), flips
    assert window_ends == E * sum(1 for s in sched if s[1])
    final = [a.final()[0] for a in ads]
    assert np.allclose(torch.exp(ad['da'][:, 1]).cpu().numpy(), final, rtol=1e-4)


def test_chain_draws_do_not_depend_on_the_ensemble_and_thinning_keeps_positions(oracle):
    from mile_amd.kernels import KERNELS
    ospec = oracle.ModelSpec(5, (16, 16, 2))
    E, T = 6, 6
    prob = oracle.synthetic_problem(ospec, 200, E, seed=5)
    eng = _engine(oracle, ospec, prob)
    ids = torch.arange(100, 100 + E, dtype=torch.int32)
    s0 = eng.nuts_init(torch.from_numpy(prob['theta0']))
    full, inf_full, kept_all = eng.nuts_step(s0, 0.01, 1.0, n_steps=T, seed=77, step_offset=40, particle_ids=ids, n_thinning=1)
    _, _, kept_thin = eng.nuts_step(s0, 0.01, 1.0, n_steps=T, seed=77, step_offset=40, particle_ids=ids, n_thinning=4)
    torch.cuda.synchronize()
    assert torch.equal(kept_thin, kept_all[[0, 4]])              # steps 40 and 44 of 40..45
    assert torch.equal(kept_all[-1], full.position)
    sub = [1, 4]
    s0s = eng.nuts_init(torch.from_numpy(prob['theta0'][sub]))
    part, inf_part, _ = eng.nuts_step(s0s, 0.01, 1.0, n_steps=T, seed=77, step_offset=40, particle_ids=ids[sub])
    torch.cuda.synchronize()
    for k in (0, 2, 3, 5):
        assert torch.equal(inf_part[k], inf_full[k][:, sub])
    assert _relerr(part.position.cpu().numpy(), full.position[sub].cpu().numpy()) < 1e-4
    # the blackjax-shaped factory
    sampler = KERNELS['nuts'](eng_target(eng, prob), step_size=0.01, inverse_mass_matrix=torch.ones(eng.d),
                              chain_ids=ids[sub])
    st = sampler.init(torch.from_numpy(prob['theta0'][sub]), 77)
    st, info = sampler.step(77, st, 40)
    torch.cuda.synchronize()
    assert info.num_integration_steps.shape == (2,) and torch.equal(info.num_integration_steps, inf_part[0][0])


def eng_target(eng, prob):
    """The unnormalised log posterior bound to the engine's data, as the trainer hands it to the sampler."""
    from mile_amd.probabilistic import ProbabilisticModel
    pm = ProbabilisticModel(eng.spec)
    return pm.bind(torch.from_numpy(prob['X']), torch.from_numpy(prob['y']))


def test_train_cli_runs_the_nuts_yaml(tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'nuts_airfoil_stock.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['experiment_name'] = 'nuts'
    cfg['training']['warmstart'].update(max_epochs=3)
    cfg['training']['sampler'].update(warmup_steps=30, n_samples=20, n_chains=3)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, str(ROOT / 'train.py'), '-c', str(tmp_path / 'cfg.yaml'), '-d', '1'],
                       capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp = tmp_path / 'nuts'
    assert not (exp / 'warmup_params.txt').exists() and not (exp / 'sampling_warmup').exists()
    assert sorted(p.name for p in (exp / 'samples').iterdir() if p.is_dir()) == ['0', '1', '2']
    assert sorted(int(p.stem.split('_')[1]) for p in (exp / 'samples' / '1').iterdir()) == list(range(20))
    info = pickle.loads((exp / 'samples' / 'info.pkl').read_bytes())
    assert set(info) == {'num_integration_steps', 'acceptance_rate', 'num_trajectory_expansions', 'is_divergent', 'energy',
                         'is_turning'}
    assert all(v.shape == (3, 20) for v in info.values())
    assert (info['num_integration_steps'] >= 1).all() and np.isfinite(info['energy']).all()
    assert 'time.sampling took' in (exp / 'training.log').read_text()
    r = subprocess.run([sys.executable, str(ROOT / 'evaluate.py'), '-e', str(exp)], capture_output=True, text=True, cwd=ROOT,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = json.loads((exp / 'metrics.json').read_text())
    assert (m['n_chains'], m['n_samples']) == (3, 20) and np.isfinite(m['lppd'])
