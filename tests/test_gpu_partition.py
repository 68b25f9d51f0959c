"""Partition sampling on the device (-m gpu): the compact gradient of every kernel AUTO can pick, MCLMC steps, the tuner and the
command-line run, against the partition target restated on the fp64 oracle (tests/partition_ref.py).  Explicit noise
throughout.  Tolerances are the project's own for the same quantities: tests/leafcheck.py per leaf for gradients, the figures
of test_gpu_parity.py::test_steps_match_oracle_explicit_noise for steps, those of
test_gpu_e2e.py::test_device_tuner_teacher_forced_against_the_fp32_oracle for the tuner."""
import math

import numpy as np
import pytest

from tests import leafcheck as L
from tests import partition_ref as PR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


def _spec(ospec):
    from mile_amd import ModelSpec
    return ModelSpec(in_features=ospec.in_features, hidden_structure=ospec.hidden_structure, activation=ospec.activation,
                     task=ospec.task, prior=ospec.prior, prior_loc=ospec.prior_loc, prior_scale=ospec.prior_scale)


def _engine(ospec, prob, frozen, kernel='auto'):
    from mile_amd.engine import Engine
    eng = Engine(_spec(ospec), torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device='cuda:0', grad_kernel=kernel)
    eng.set_partition(torch.from_numpy(frozen))
    return eng


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _problem(oracle, ospec, N, E, seed):
    """Data, frozen rows that differ per chain, and a compact point drawn separately (so the merged net is neither)."""
    prob = oracle.synthetic_problem(ospec, N, E, seed=seed)
    frozen = prob['theta0'].astype(np.float32)
    other = oracle.synthetic_problem(ospec, N, E, seed=seed + 100)['theta0'].astype(np.float32)
    compact = PR.partition(ospec, other)
    assert not np.array_equal(frozen[0], frozen[-1])
    if ospec.activation == 'relu':
        # rows with a pre-activation within fp32 rounding of the ReLU kink may fall on either side in fp32 and fp64: left
        # out for the oracle and the device alike (as tests/test_gpu_parity.py::test_logpost_grad_matches_oracle does)
        full = PR.merge(ospec, compact, frozen).astype(np.float64)
        _, zs, _ = oracle.mlp_forward(ospec, full, prob['X'], keep=True)
        near = np.zeros(N, dtype=bool)
        for z in zs[:-1]:
            near |= (np.abs(z) < 3e-7 * np.abs(z).max()).any(axis=(0, 2))
        assert near.sum() <= 17
        if near.any():
            prob = dict(prob, X=np.ascontiguousarray(prob['X'][~near]), y=np.ascontiguousarray(prob['y'][~near]))
    return prob, frozen, compact


GRAD_CASES = [
    # F, hidden, activation, task, prior, N, E, kernels, what AUTO resolves to (its own priority list, unchanged by the mode)
    (8, (16,) * 8 + (2,), 'relu', 'regr', 'Normal', 100, 5, ('auto', 'mfma_narrow_f32', 'generic'), 'mfma_narrow_f32'),   # fused, deep-narrow form
    (5, (16, 16, 2), 'relu', 'regr', 'Normal', 70, 3, ('auto', 'generic'), 'mfma_narrow_f32'),                              # fused, register weights
    (5, (16, 16, 2), 'relu', 'regr', 'Laplace', 70, 3, ('auto', 'generic'), 'mfma_narrow_f32'),                             # the other prior
    (7, (40, 40, 3), 'tanh', 'classification', 'Normal', 130, 4, ('auto', 'generic'), 'mfma_narrow_f32'),                   # fused, LDS weights, softmax head
    (5, (64, 64, 64, 2), 'relu', 'regr', 'Normal', 300, 6, ('generic', 'mfma_w64', 'mfma_w64_bf16x3', 'auto'), 'mfma_w64_bf16x3'),   # general path
    (9, (128, 128, 2), 'relu', 'regr', 'Normal', 192, 4, ('mfma_wide_bf16x3', 'auto'), 'mfma_wide_bf16x3'),
    (4, (8,) * 11 + (2,), 'tanh', 'regr', 'Normal', 75, 3, ('generic',), None),                               # 12 layers: split segments
]


@pytest.mark.parametrize('F,hs,act,task,prior,N,E,kernels,auto', GRAD_CASES)
def test_compact_gradient_matches_partition_ref(oracle, F, hs, act, task, prior, N, E, kernels, auto):
    ospec = oracle.ModelSpec(F, hs, activation=act, task=task, prior=prior, prior_scale=0.7 if prior == 'Laplace' else 1.0)
    prob, frozen, compact = _problem(oracle, ospec, N, E, seed=3)
    f = PR.logdensity_and_grad(ospec, frozen, prob['X'], prob['y'])
    lp_ref, g_ref = f(compact.astype(np.float64))
    _, g32 = f(compact)                                                   # the float32 restatement's own error
    leaves = PR.compact_leaves(ospec)
    d_s = len(PR.index(ospec))
    assert g_ref.shape == (E, d_s) and leaves[-1][2] == d_s
    bound = L.leaf_bounds(leaves, E, g32=g32, g_ref=g_ref)
    for k in kernels:
        eng = _engine(ospec, prob, frozen, k)
        assert eng.dim == d_s and eng.d == ospec.n_params
        assert eng.partition_segments == [(b, e - b) for b, e in PR.segments(ospec)]
        if k == 'auto':   # AUTO keeps its choice in partition mode: the fused kernel wherever it picks k_grad_narrow
            assert eng.grad_kernel == auto, (eng.grad_kernel, auto)
            if auto == 'mfma_narrow_f32':
                assert 'k_grad_narrow<partition>' == eng.grad_launch_info(E)['kernel']
        lp, g = eng.logpost_grad(torch.from_numpy(compact))
        torch.cuda.synchronize()
        g, lp = g.cpu().numpy(), lp.cpu().numpy()
        assert g.shape == (E, d_s)
        err = L.leaf_errors(g, g_ref, leaves)
        print(f'{k} F={F} {hs} {prior}: logp {_relerr(lp, lp_ref):.2e}, worst leaf {err.max():.2e} (bound {bound.min():.1e})')
        assert _relerr(lp, lp_ref) < 2e-5, k
        L.assert_leaves(g, g_ref, leaves, bound=bound, tag=(k, F, hs, act, prior))
        # merge / partition on the device agree with the layout of the reference side
        assert np.array_equal(eng.merge(torch.from_numpy(compact)).cpu().numpy(), PR.merge(ospec, compact, frozen))
        assert np.array_equal(eng.partition(torch.from_numpy(frozen)).cpu().numpy(), PR.partition(ospec, frozen))


@pytest.mark.parametrize('refresh', ['O-step-O', 'step-O'])
@pytest.mark.parametrize('F,hs,N,kernel', [(8, (16,) * 8 + (2,), 100, 'auto'), (5, (64, 64, 64, 2), 300, 'auto')])
def test_steps_match_oracle_on_the_partition_target(oracle, F, hs, N, kernel, refresh):
    ospec = oracle.ModelSpec(F, hs)
    E, T = 6, 10
    prob, frozen, compact = _problem(oracle, ospec, N, E, seed=11)
    d_s = compact.shape[1]
    rng = np.random.default_rng(5)
    z0 = rng.standard_normal((E, d_s)).astype(np.float32)
    noise = rng.standard_normal((T, 2, E, d_s)).astype(np.float32)
    f = PR.logdensity_and_grad(ospec, frozen, prob['X'], prob['y'])
    st = oracle.mclmc_init(f, compact.astype(np.float64), z0.astype(np.float64))
    infos, kept = [], []
    for i in range(T):
        st, info = oracle.mclmc_step(f, st, prob['eps'].astype(np.float64), prob['L'].astype(np.float64),
                                     noise[i, 0].astype(np.float64), noise[i, 1].astype(np.float64), refresh=refresh)
        infos.append(info)
        if i % 3 == 0:
            kept.append(st.position.copy())
    eng = _engine(ospec, prob, frozen, kernel)
    assert eng.grad_kernel == ('mfma_narrow_f32' if hs[0] == 16 else 'mfma_w64_bf16x3')
    s0 = eng.init(torch.from_numpy(compact), noise=torch.from_numpy(z0))
    s1, info, samples = eng.step(s0, torch.from_numpy(prob['eps']), torch.from_numpy(prob['L']), n_steps=T,
                                 noise=torch.from_numpy(noise), n_thinning=3, refresh=refresh)
    torch.cuda.synchronize()
    assert s1.position.shape == (E, d_s)
    assert _relerr(s1.position.cpu().numpy(), st.position) < 1e-4
    assert np.abs(s1.momentum.cpu().numpy() - st.momentum).max() < 1e-4 * np.abs(st.momentum).max() + 1e-6
    assert _relerr(s1.logdensity.cpu().numpy(), st.logdensity) < 1e-5
    assert _relerr(s1.logdensity_grad.cpu().numpy(), st.logdensity_grad) < 1e-3
    assert np.abs(np.linalg.norm(s1.momentum.cpu().numpy().astype(np.float64), axis=1) - 1).max() < 1e-5
    dE = np.stack([i.energy_change for i in infos])
    dK = np.stack([i.kinetic_change for i in infos])
    assert np.abs(info.kinetic_change.cpu().numpy() - dK).max() < 1e-3 + 1e-3 * np.abs(dK).max()
    assert np.abs(info.energy_change.cpu().numpy() - dE).max() < 5e-2
    assert samples.shape == (4, E, d_s)
    assert _relerr(samples.cpu().numpy(), np.stack(kept)) < 1e-4
    assert torch.equal(s0.position.cpu(), torch.from_numpy(compact))          # the input state was not modified
    # the merged samples carry the frozen rows bit for bit
    merged = eng.merge(samples).cpu().numpy()
    hidden = np.setdiff1d(np.arange(ospec.n_params), PR.index(ospec))
    assert merged.shape == (4, E, ospec.n_params)
    assert np.array_equal(merged[..., hidden], np.broadcast_to(frozen[:, hidden], (4, E, len(hidden))))


def _to_dev_state(st):
    from mile_amd.engine import IntegratorState
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    return IntegratorState(f(st.position), f(st.momentum), f(st.logdensity), f(st.logdensity_grad))


def test_tuner_teacher_forced_with_the_compact_dimension(oracle):
    """30 + 10 steps of make_L_step_size_adaptation (phases 1 + 2) run by the ORACLE in float32 on the partition target --
    tuner_step, what tune_phase12 loops over, takes its dimension from the state: dim = d_s -- and at each step the device does
    ONE mile_tune step from the oracle's state, step size and adaptive state on the same noise (the method and the figures of
    test_gpu_e2e.py::test_device_tuner_teacher_forced_against_the_fp32_oracle).  On the steps whose energy change is resolved
    the device's new step size must also be FAR from what dim = d_full gives in the oracle (tests/test_partition_host.py::
    test_tuner_step_size_depends_on_the_dimension shows the two differ by ~50 %), so a tuner run with the wrong dimension fails."""
    ospec = oracle.ModelSpec(8, (16,) * 8 + (2,))
    E, N = 3, 100
    prob, frozen, compact = _problem(oracle, ospec, N, E, seed=21)
    d_s, d_full = compact.shape[1], ospec.n_params
    rng = np.random.default_rng(7)
    t1, t2 = 30, 10
    f32 = np.float32
    z0 = rng.standard_normal((E, d_s)).astype(f32)
    noise = rng.standard_normal((t1 + t2, 2, E, d_s)).astype(f32)
    f = PR.logdensity_and_grad(ospec, frozen, prob['X'].astype(f32), prob['y'].astype(f32))
    v0, v1, trust, n_eff = 0.5, 0.1, 1.5, 100
    decay = f32((n_eff - 1.0) / (n_eff + 1.0))
    total = t1 + t2 + 1
    eng = _engine(ospec, prob, frozen)
    assert eng.grad_kernel == 'mfma_narrow_f32'
    st = oracle.mclmc_init(f, compact.astype(f32), z0)
    Lv = np.full(E, max(math.sqrt(d_s), 15.0), f32)               # warmup.py:205 with d = d_s
    eps = np.full(E, 0.05, f32)     # (from 0.01 the float32 ORACLE resolves no energy change in 40 steps on this target; from 0.05, 116 of 120)
    sdc = np.ones((E, d_s), f32)
    kw = dict(desired_energy_var_start=v0, desired_energy_var_end=v1, trust_in_estimate=trust, decay_rate=float(decay))
    ad = oracle.AdaptiveState.fresh(E, d_s, f32)
    masks = [1.0] * t1 + [0.0] * t2
    resolved = n_checked = told_apart = 0
    for i, mask in enumerate(masks):
        z = noise[i]
        dst = _to_dev_state(st)
        tuner = {k: torch.from_numpy(np.ascontiguousarray(v, f32)).cuda() for k, v in
                 dict(step_size=eps, step_size_max=ad.step_size_max, time=ad.time, x_average=ad.x_average,
                      stream_weight=ad.W, stream_average=ad.avg).items()}
        info_d = eng.tune(dst, tuner, torch.from_numpy(Lv), 1, schedule_step0=i, n_mask_steps=t1, schedule_total=total,
                          noise=torch.from_numpy(z[None]), want_info=True, **kw)
        torch.cuda.synchronize()
        ad_in = ad.copy()
        var = oracle.desired_energy_var(i, total, v0, v1)
        st_n, eps_n, ok, info = oracle.tuner_step(f, st, eps, Lv, sdc, z[0], z[1], ad, mask=mask, var=var,
                                                  trust_in_estimate=trust, decay=decay)
        assert ok.all()
        where = f'step {i}'
        assert _relerr(dst.position.cpu(), st_n.position) < 2e-5, where
        assert np.abs(dst.momentum.cpu().numpy() - st_n.momentum).max() < 2e-5, where
        assert _relerr(dst.logdensity.cpu(), st_n.logdensity) < 2e-6, where
        dE_d = info_d.energy_change[0].cpu().numpy()
        ulp = float(np.spacing(f32(np.abs(st_n.logdensity).max())))
        assert np.abs(dE_d - info.energy_change).max() <= 16 * ulp + 1e-4 * np.abs(info.energy_change).max(), where
        chk = ad_in.copy()
        chk.step_size_max = np.nan_to_num(chk.step_size_max)
        eps_chk, _, _ = oracle.predictor_update(dE_d.astype(f32), eps, chk, dim=d_s, var=var, trust_in_estimate=trust, decay=decay)
        got = tuner['step_size'].cpu().numpy()
        assert _relerr(got, eps_chk) < 2e-5, where
        assert _relerr(tuner['x_average'].cpu(), chk.x_average) < 2e-5 and _relerr(tuner['time'].cpu(), chk.time) < 2e-5, where
        if mask == 0.0:
            assert _relerr(tuner['stream_weight'].cpu(), ad_in.W + got) < 2e-5, where
            assert tuner['stream_average'].shape == (E, 2, d_s)
            assert _relerr(tuner['stream_average'].cpu(), ad.avg) < 2e-5 + 2 * _relerr(got, eps_n), where
        good = np.abs(info.energy_change) > 100 * ulp
        n_checked += E
        resolved += int(good.sum())
        if good.any():
            assert np.abs(got - eps_n)[good].max() / eps_n[good].max() < 1e-3, where
            # the same predictor with the FULL dimension, from the same inputs: not what the device computed
            wrong = ad_in.copy()
            wrong.step_size_max = np.nan_to_num(wrong.step_size_max)
            eps_wrong, _, _ = oracle.predictor_update(info.energy_change.astype(f32), eps, wrong, dim=d_full, var=var,
                                                      trust_in_estimate=trust, decay=decay)
            apart = np.abs(eps_wrong - eps_n)[good] / eps_n[good] > 1e-3
            told_apart += int(apart.sum())
            assert np.all(np.abs(got - eps_wrong)[good][apart] / eps_n[good][apart] > 1e-3), where
        st, eps = st_n, eps_n
    assert resolved >= 0.5 * n_checked, (resolved, n_checked)
    assert told_apart >= 0.5 * resolved, (told_apart, resolved)    # the dimension was visible on most resolved steps
    var_x = ad.avg[:, 1] - np.square(ad.avg[:, 0])
    assert var_x.shape == (E, d_s) and np.all(var_x.sum(axis=1) > 0)


def test_refusals(oracle):
    from mile_amd import _lib
    from mile_amd.engine import Engine, HMCState
    from mile_amd.spec import LeNettiSpec
    rng = np.random.default_rng(0)
    spec = LeNettiSpec(channels=1, height=8, width=8, out_dim=3)
    X = rng.standard_normal((20, 64)).astype(np.float32)
    y = rng.integers(0, 3, 20)
    eng = Engine(spec, torch.from_numpy(X), torch.from_numpy(y), device='cuda:0')
    with pytest.raises(_lib.MileHipError, match='error -1.*FCN only'):
        eng.set_partition(torch.zeros(2, eng.d))
    assert eng.dim == eng.d and not eng.partitioned
    # NUTS on a handle in partition mode
    ospec = oracle.ModelSpec(5, (16, 16, 2))
    prob, frozen, compact = _problem(oracle, ospec, 70, 3, seed=3)
    eng = _engine(ospec, prob, frozen)
    with pytest.raises(_lib.MileHipError, match='error -1.*NUTS is not built'):
        eng.nuts_reserve(3, 3)
    import ctypes as C
    sc, a = _lib.StateC(), _lib.NutsArgsC()
    full = torch.from_numpy(frozen).cuda()
    lp = torch.zeros(3, device='cuda')
    sc.n_particles, sc.position, sc.logdensity, sc.logdensity_grad = 3, full.data_ptr(), lp.data_ptr(), full.data_ptr()
    assert eng.lib.mile_nuts_step(eng._h, C.byref(sc), C.byref(a), None) == -1
    assert b'NUTS is not built' in eng.lib.mile_last_error()
    # E different from the frozen rows'
    with pytest.raises(_lib.MileHipError, match="error -1.*E differs from the frozen rows'"):
        eng.logpost_grad(torch.from_numpy(compact[:2]))
    # a net without a frozen layer: accepted, ordinary sampling
    o2 = oracle.ModelSpec(5, (16, 2))
    p2 = oracle.synthetic_problem(o2, 70, 3, seed=3)
    e2 = _engine(o2, p2, p2['theta0'])
    assert e2.partitioned and e2.dim == e2.d and e2.partition_segments == []
    lp, g = e2.logpost_grad(torch.from_numpy(p2['theta0']))
    lp_ref, g_ref = oracle.logpost_and_grad(o2, p2['theta0'].astype(np.float64), p2['X'], p2['y'])
    assert _relerr(lp.cpu().numpy(), lp_ref) < 2e-5 and _relerr(g.cpu().numpy(), g_ref) < 2e-5


def test_train_and_evaluate_cli(tmp_path):
    """`train.py -c` on experiments/mclmc_partition_synthetic.yaml cut to a few hundred steps, then `evaluate.py`."""
    import json
    import subprocess
    import sys
    from pathlib import Path

    import yaml
    root = Path(__file__).resolve().parents[1]
    cfg = yaml.safe_load((root / 'experiments' / 'mclmc_partition_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['experiment_name'] = 'part_small'
    cfg['training']['warmstart'].update(max_epochs=3, patience=2)
    cfg['training']['sampler'].update(warmup_steps=200, n_samples=100, n_chains=4, n_thinning=10)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, str(root / 'train.py'), '-c', str(tmp_path / 'cfg.yaml'), '-d', '1'],
                       capture_output=True, text=True, cwd=root, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp = tmp_path / 'part_small'
    lines = (exp / 'warmup_params.txt').read_text().splitlines()
    assert len(lines) == 2 and all(len(l.split(',')) == 4 and np.all(np.isfinite(np.array(l.split(','), float))) for l in lines)
    keys = [f'fcn.layer{i}.{k}' for i in range(9) for k in ('bias', 'kernel')]
    for c in range(4):
        ws = np.load(exp / 'warmstart' / f'params_{c}.npz')
        files = sorted((exp / 'samples' / str(c)).glob('sample_*.npz'), key=lambda p: int(p.stem.split('_')[1]))
        assert [p.name for p in files] == [f'sample_{n}.npz' for n in range(0, 100, 10)]
        first, last = np.load(files[0]), np.load(files[-1])
        for p in files:
            z = np.load(p)
            assert z.files == keys == ws.files
            for k in keys:
                assert z[k].shape == ws[k].shape and z[k].dtype == ws[k].dtype and np.isfinite(z[k]).all()
                if k.split('.')[1] not in ('layer0', 'layer8'):
                    assert np.array_equal(z[k], ws[k]), (c, p.name, k)          # hidden layers: the warm-start member's
        for k in ('fcn.layer0.bias', 'fcn.layer0.kernel', 'fcn.layer8.bias', 'fcn.layer8.kernel'):
            assert not np.array_equal(first[k], last[k]), (c, k)
    r = subprocess.run([sys.executable, str(root / 'evaluate.py'), '-e', str(exp), '--split', 'valid'], capture_output=True,
                       text=True, cwd=root, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = json.loads((exp / 'metrics.json').read_text())
    assert m['split'] == 'valid' and np.isfinite(m['lppd'])
