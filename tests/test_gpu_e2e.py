"""GPU tests of the path around the kernels: golden vectors through the C ABI, sharding
independence, the tuner, inference_loop's files, the CLI and the LPPD gate (-m gpu)."""
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

ROOT = Path(__file__).resolve().parents[1]
GOLD = Path(__file__).parent / 'golden'


def _spec(ospec):
    from mile_amd import ModelSpec
    return ModelSpec(in_features=ospec.in_features, hidden_structure=ospec.hidden_structure,
                     activation=ospec.activation, task=ospec.task, prior=ospec.prior,
                     prior_loc=ospec.prior_loc, prior_scale=ospec.prior_scale)


def _engine(ospec, X, y, kernel='auto'):
    from mile_amd.engine import Engine
    return Engine(_spec(ospec), torch.from_numpy(np.asarray(X)), torch.from_numpy(np.asarray(y)), device='cuda:0',
                  grad_kernel=kernel)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize('name,hs,F,kw,refresh,kernels', [
    ('regr_relu_8x8', (8, 8, 2), 5, {}, 'O-step-O', ('generic',)),
    ('regr_relu_8x8_stepO', (8, 8, 2), 5, {}, 'step-O', ('generic',)),
    ('class_tanh_6x4', (6, 4), 7, dict(activation='tanh', task='classification', prior='Laplace', prior_scale=0.5),
     'O-step-O', ('generic',)),
    ('regr_relu_64x3', (64, 64, 64, 2), 5, {}, 'O-step-O', ('generic', 'mfma_w64', 'mfma_w64_bf16x3')),
])
def test_hip_reproduces_golden_vectors(oracle, name, hs, F, kw, refresh, kernels):
    z = np.load(GOLD / f'{name}.npz')
    ospec = oracle.ModelSpec(F, hs, **kw)
    T = z['noise'].shape[0]
    for k in kernels:
        eng = _engine(ospec, z['X'], z['y'], k)
        s0 = eng.init(torch.from_numpy(z['theta0']), noise=torch.from_numpy(z['z0']))
        assert _rel(s0.logdensity.cpu(), z['logp0']) < 1e-5 and _rel(s0.logdensity_grad.cpu(), z['grad0']) < 2e-5
        assert np.abs(s0.momentum.cpu().numpy() - z['u0']).max() < 1e-6
        s1, info, _ = eng.step(s0, torch.from_numpy(z['eps']), torch.from_numpy(z['L']), n_steps=1,
                               noise=torch.from_numpy(z['noise'][:1]), refresh=refresh)
        assert _rel(s1.position.cpu(), z['x_1']) < 1e-5 and np.abs(s1.momentum.cpu().numpy() - z['u_1']).max() < 2e-5
        sT, info, _ = eng.step(s0, torch.from_numpy(z['eps']), torch.from_numpy(z['L']), n_steps=T,
                               noise=torch.from_numpy(z['noise']), refresh=refresh)
        # fp32 vs the fp64 golden trajectory: 1e-4 after <= 10 steps
        assert _rel(sT.position.cpu(), z[f'x_{T}']) < 1e-4
        assert np.abs(sT.momentum.cpu().numpy() - z[f'u_{T}']).max() < 1e-3 * np.abs(z[f'u_{T}']).max()
        assert _rel(sT.logdensity.cpu(), z[f'logp_{T}']) < 1e-4
        got = torch.stack([info.logdensity, info.kinetic_change, info.energy_change], -1).cpu().numpy()
        assert np.abs(got[..., 0] - z['info'][..., 0]).max() < 1e-4 * np.abs(z['info'][..., 0]).max()
        assert np.abs(got[..., 1] - z['info'][..., 1]).max() < 2e-3 + 1e-3 * np.abs(z['info'][..., 1]).max()
        assert np.abs(got[..., 2] - z['info'][..., 2]).max() < 2e-2


def test_results_do_not_depend_on_sharding(oracle):
    """Counter RNG keyed by GLOBAL particle id: 8 particles in one ensemble == two shards of 4, bit for bit."""
    ospec = oracle.ModelSpec(5, (64, 64, 64, 2))
    prob = oracle.synthetic_problem(ospec, 200, 8, seed=7)
    eng = _engine(ospec, prob['X'], prob['y'])
    th, eps, L = (torch.from_numpy(prob[k]) for k in ('theta0', 'eps', 'L'))
    ids = torch.arange(100, 108, dtype=torch.int32)

    def run(sl):
        s = eng.init(th[sl], seed=99, particle_ids=ids[sl])
        s, info, kept = eng.step(s, eps[sl], L[sl], n_steps=7, seed=99, step_offset=3, n_thinning=2, particle_ids=ids[sl])
        return s, info, kept
    full, inf_f, kept_f = run(slice(0, 8))
    a, inf_a, kept_a = run(slice(0, 4))
    b, inf_b, kept_b = run(slice(4, 8))
    assert torch.equal(full.position, torch.cat([a.position, b.position]))
    assert torch.equal(full.momentum, torch.cat([a.momentum, b.momentum]))
    assert torch.equal(kept_f, torch.cat([kept_a, kept_b], dim=1))
    assert kept_f.shape[0] == 3                      # global steps 3..9: kept 4, 6, 8
    assert torch.equal(inf_f.energy_change, torch.cat([inf_a.energy_change, inf_b.energy_change], dim=1))
    # and a different seed gives a different trajectory
    s2 = eng.init(th[:4], seed=100, particle_ids=ids[:4])
    assert not torch.equal(s2.momentum, eng.init(th[:4], seed=99, particle_ids=ids[:4]).momentum)


@pytest.mark.parametrize('F,hs', [(5, (7, 6, 2)), (4, (8, 6, 2)), (5, (64, 64, 64, 2))])   # d odd / d % 4 == 0 / d % 4 == 2
def test_preconditioned_steps_and_alignment_paths(oracle, F, hs):
    ospec = oracle.ModelSpec(F, hs)
    d = ospec.n_params
    E, T = 3, 4
    prob = oracle.synthetic_problem(ospec, 50, E, seed=13)
    rng = np.random.default_rng(1)
    sdc = (0.5 + rng.random((E, d))).astype(np.float32)
    z0 = rng.standard_normal((E, d)).astype(np.float32)
    noise = rng.standard_normal((T, 2, E, d)).astype(np.float32)
    f = lambda th: oracle.logpost_and_grad(ospec, th, prob['X'], prob['y'])
    st = oracle.mclmc_init(f, prob['theta0'].astype(np.float64), z0.astype(np.float64))
    for i in range(T):
        st, _ = oracle.mclmc_step(f, st, prob['eps'].astype(np.float64), prob['L'].astype(np.float64),
                                  noise[i, 0].astype(np.float64), noise[i, 1].astype(np.float64),
                                  sqrt_diag_cov=sdc.astype(np.float64))
    eng = _engine(ospec, prob['X'], prob['y'])
    s = eng.init(torch.from_numpy(prob['theta0']), noise=torch.from_numpy(z0))
    s, _, _ = eng.step(s, torch.from_numpy(prob['eps']), torch.from_numpy(prob['L']), n_steps=T,
                       noise=torch.from_numpy(noise), sqrt_diag_cov=torch.from_numpy(sdc))
    assert _rel(s.position.cpu(), st.position) < 1e-4
    assert np.abs(s.momentum.cpu().numpy() - st.momentum).max() < 1e-4


@pytest.mark.parametrize('F,hs,sdc', [(9, (128, 128, 2), False), (7, (129, 127, 2), True), (16, (128, 128, 128, 2), False),
                                      (9, (192, 192, 2), False), (11, (190, 203, 2), True)])
def test_update_kernel_beyond_the_register_cache_matches_the_two_pass_form(oracle, monkeypatch, F, hs, sdc):
    """16384 < d <= 36864 (B3: 34562): `k_update_big` -- u in registers, g parked in LDS, noise generated twice -- and beyond
    that `k_update_seg` (segments of 8192 elements on all CUs), against the two-pass `k_update` on the same Philox streams: same trajectory up to fp32 summation order, same
    kept samples, unit momentum.  Cases: NK = 5 (16-byte rows), d % 4 == 2 with a preconditioner, NK = 9 (B3's d)."""
    ospec = oracle.ModelSpec(F, hs)
    d = ospec.n_params
    assert d > 16384              # <= 36864: k_update_big; beyond: the segmented k_update_seg (all CUs), d = 39362 and 41461 (odd)
    E, T = 5, 6
    prob = oracle.synthetic_problem(ospec, 96, E, seed=21)
    rng = np.random.default_rng(2)
    kw = dict(n_steps=T, seed=11, n_thinning=2, particle_ids=torch.arange(E, dtype=torch.int32))
    if sdc:
        kw['sqrt_diag_cov'] = torch.from_numpy((0.5 + rng.random((E, d))).astype(np.float32))
    eps, L = torch.from_numpy(prob['eps']), torch.from_numpy(prob['L'])
    out = {}
    for two_pass in (False, True):
        if two_pass:
            monkeypatch.setenv('MILE_NO_UPD_BIG', '1')
            monkeypatch.setenv('MILE_NO_UPD_SEG', '1')
        eng = _engine(ospec, prob['X'], prob['y'], 'generic')
        s0 = eng.init(torch.from_numpy(prob['theta0']), seed=11, particle_ids=kw['particle_ids'])
        out[two_pass] = eng.step(s0, eps, L, **kw)
    (sa, ia, ka), (sb, ib, kb) = out[False], out[True]
    assert _rel(sa.position.cpu(), sb.position.cpu()) < 2e-5
    assert np.abs(sa.momentum.cpu().numpy() - sb.momentum.cpu().numpy()).max() < 2e-5
    assert _rel(ka.cpu(), kb.cpu()) < 2e-5
    assert _rel(sa.logdensity.cpu(), sb.logdensity.cpu()) < 1e-5
    ulp = float(np.spacing(np.float32(sb.logdensity.abs().max().item())))   # energy_change carries a difference of log-densities
    assert np.abs(ia.energy_change.cpu().numpy() - ib.energy_change.cpu().numpy()).max() <= 4 * ulp + 1e-5
    assert (sa.momentum.double().norm(dim=1) - 1).abs().max().item() < 1e-5 or sdc


def test_kernel_registry_factory_has_blackjax_shape(oracle):
    from mile_amd.kernels import KERNELS
    from mile_amd.probabilistic import ProbabilisticModel
    from mile_amd.tree import PRNGKey, unravel_tree
    ospec = oracle.ModelSpec(5, (16, 16, 2))
    prob = oracle.synthetic_problem(ospec, 120, 3, seed=3)
    pm = ProbabilisticModel(_spec(ospec), task='regr')
    x, y = torch.from_numpy(prob['X']), torch.from_numpy(prob['y'])
    log_post = pm.bind(x, y)
    sampler = KERNELS['mclmc'](log_post, L=torch.from_numpy(prob['L']), step_size=torch.from_numpy(prob['eps']))
    tree = unravel_tree(pm.spec, torch.from_numpy(prob['theta0']))          # the reference passes a param tree
    key = PRNGKey(5)
    state = sampler.init(tree, key)
    new, info = sampler.step(key, state)
    # same step on the oracle with the noise the device drew
    ids = np.arange(3)
    f = lambda th: oracle.logpost_and_grad(ospec, th, prob['X'], prob['y'])
    zi = oracle.philox_normal(key.seed, ids, 0, 2, ospec.n_params)
    st = oracle.mclmc_init(f, prob['theta0'].astype(np.float64), zi)
    st, oinfo = oracle.mclmc_step(f, st, prob['eps'].astype(np.float64), prob['L'].astype(np.float64),
                                  oracle.philox_normal(key.seed, ids, 0, 0, ospec.n_params),
                                  oracle.philox_normal(key.seed, ids, 0, 1, ospec.n_params))
    assert _rel(new.position.cpu(), st.position) < 1e-5
    assert _rel(info.logdensity.cpu(), oinfo.logdensity) < 1e-5
    assert info.energy_change.shape == (3,)
    assert torch.equal(state.position.cpu(), torch.from_numpy(prob['theta0']))   # step did not mutate its input
    lp = pm.log_unnormalized_posterior(tree, x, y)
    assert _rel(lp.cpu(), oracle.logpost_and_grad(ospec, prob['theta0'].astype(np.float64), prob['X'], prob['y'])[0]) < 1e-5


def test_warmup_tuner_matches_oracle_with_explicit_noise(oracle):
    from mile_amd.warmup import mclmc_find_L_and_step_size
    ospec = oracle.ModelSpec(5, (8, 8, 2))
    E, d = 3, ospec.n_params
    prob = oracle.synthetic_problem(ospec, 60, E, seed=21)
    rng = np.random.default_rng(2)
    # short horizon: the adaptation amplifies fp32 rounding of the energy error (the oracle run in
    # fp32 drifts 5-40 % from its own fp64 run after 50 adaptive steps, < 0.5 % after 10)
    t1, t2, t3 = 8, 3, 4
    z0 = rng.standard_normal((E, d)).astype(np.float32)
    noise12 = rng.standard_normal((t1 + t2, 2, E, d)).astype(np.float32)
    noise3 = rng.standard_normal((t3, 2, E, d)).astype(np.float32)
    f = lambda th: oracle.logpost_and_grad(ospec, th, prob['X'], prob['y'])
    kw = dict(step_size_init=0.01, desired_energy_var_start=0.5, desired_energy_var_end=0.1, trust_in_estimate=1.5,
              num_effective_samples=100)
    st = oracle.mclmc_init(f, prob['theta0'].astype(np.float64), z0.astype(np.float64))
    res = oracle.tune_phase12(f, st, lambda i: (noise12[i, 0].astype(np.float64), noise12[i, 1].astype(np.float64)),
                              t1, t2, record=True, **kw)
    st3, L3 = oracle.tune_phase3(f, res.state, res.step_size, res.L,
                                 lambda i: (noise3[i, 0].astype(np.float64), noise3[i, 1].astype(np.float64)), t3)
    eng = _engine(ospec, prob['X'], prob['y'])
    s0 = eng.init(torch.from_numpy(prob['theta0']), noise=torch.from_numpy(z0))
    n12, n3 = torch.from_numpy(noise12).cuda(), torch.from_numpy(noise3).cuda()
    state, params = mclmc_find_L_and_step_size(
        eng, s0, 0, tune1_steps=t1, tune2_steps=t2, tune3_steps=t3, diagonal_preconditioning=False,
        noise_fn=lambda i: n12[i] if i < 10 ** 9 else n3[i - 10 ** 9], **kw)
    assert _rel(params.step_size.cpu(), res.step_size) < 2e-2
    assert _rel(params.L.cpu(), L3) < 5e-2
    assert _rel(state.position.cpu(), st3.position) < 2e-2
    assert params.sqrt_diag_cov.shape == (E, d) and torch.all(params.sqrt_diag_cov == 1)
    # diagonal_preconditioning with d = 138 < 225: the re-adjustment steps run with the phase-1 L = 15, not sqrt(d) = 11.7
    # (src/training/warmup.py:389-403); t2 = 6 -> two extra steps.  WHICH L those steps use is pinned exactly on the CPU
    # (tests/test_host.py::test_readjustment_runs_with_the_phase1_L_and_returns_sqrt_dim, tests/test_oracle.py::
    # test_tuner_readjustment_keeps_phase1_L).  Here: both device forms of the branch agree with each other, return
    # sqrt(d), and track the fp64 oracle -- loosely, because within these few steps the predictor multiplies the step size
    # by two orders of magnitude (xi ~ dE^2 is tiny at first) and fp32 / fp64 trajectories part ways (measured 20-60 %).
    assert d < 225
    t1, t2 = 8, 6
    kw = dict(kw, step_size_init=0.02, desired_energy_var_start=5e-4, desired_energy_var_end=1e-4)
    noise_d = rng.standard_normal((t1 + t2 + t2 // 3, 2, E, d)).astype(np.float32)
    st = oracle.mclmc_init(f, prob['theta0'].astype(np.float64), z0.astype(np.float64))
    res = oracle.tune_phase12(f, st, lambda i: (noise_d[i, 0].astype(np.float64), noise_d[i, 1].astype(np.float64)),
                              t1, t2, diagonal_preconditioning=True, **kw)
    nd = torch.from_numpy(noise_d).cuda()
    got = {}
    for host in (False, True):
        s0 = eng.init(torch.from_numpy(prob['theta0']), noise=torch.from_numpy(z0))
        state, params = mclmc_find_L_and_step_size(eng, s0, 0, tune1_steps=t1, tune2_steps=t2, tune3_steps=0,
                                                   diagonal_preconditioning=True, noise_fn=lambda i: nd[i],
                                                   force_host_loop=host, **kw)
        assert torch.allclose(params.L.cpu(), torch.full((E,), math.sqrt(d)))
        got[host] = params
        print(f'diag-precond d={d} host_loop={host}: eps {params.step_size.cpu().numpy()} oracle {res.step_size}')
    sd_o = res.sqrt_diag_cov
    good = np.isfinite(sd_o) & (sd_o > 0.05 * np.nanmax(sd_o))
    for host in (False, True):
        sd_d = got[host].sqrt_diag_cov.cpu().numpy()
        assert good.mean() > 0.5 and np.abs(sd_d[good] - sd_o[good]).max() / sd_o[good].max() < 0.25, host
        # free-running fp32 vs fp64 through 16 adaptive steps that move eps by two orders of magnitude: a sanity bound only --
        # the step-for-step statement is test_device_tuner_teacher_forced_against_the_fp32_oracle[True-False]
        assert np.all(np.abs(np.log(got[host].step_size.cpu().numpy() / res.step_size)) < math.log(6.0)), host
    assert _rel(got[False].step_size.cpu(), got[True].step_size.cpu()) < 5e-2
    assert _rel(got[False].sqrt_diag_cov.cpu(), got[True].sqrt_diag_cov.cpu()) < 2e-2


def _to_dev_state(st):
    from mile_amd.engine import IntegratorState
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    return IntegratorState(f(st.position), f(st.momentum), f(st.logdensity), f(st.logdensity_grad))


@pytest.mark.parametrize('diag,post', [(False, False), (True, False), (False, True)])
def test_device_tuner_teacher_forced_against_the_fp32_oracle(oracle, monkeypatch, diag, post):
    """VERDICT r2 item 2.  A free-running fp32 tuner cannot be held to 1e-3 over >= 50 adaptive steps by ANY second fp32
    implementation: xi ~ dE^2 with dE a difference of O(1e2..1e4) log-densities, and the oracle run in float32 moves 20-50 %
    in step size when its start is perturbed by 1e-7 (profiles/r03/03_tuner_sensitivity.md).  So every step is checked on its
    own instead: the ORACLE runs the adaptive loop in float32 (make_L_step_size_adaptation, warmup.py:271-363; 48 + 18 steps,
    and with diagonal_preconditioning the 6 re-adjustment steps under the tune-2 preconditioner), and at each step the device
    gets the oracle's state, step size and adaptive state, does ONE mile_tune step on the same noise, and must reproduce
      * the kernel step: position / momentum 2e-5, logdensity 2e-6, energy_change to a few ulps of the log-density;
      * the predictor GIVEN ITS OWN energy change -- xi, weight, x_average, time, step size, step_size_max as the
        reference writes them (warmup.py:301-326) -- to 2e-5;
      * the streaming averages of x and x^2 (warmup.py:343-348) to 2e-5;
      * and the oracle's next step size itself to 1e-3 wherever the energy change is resolved (|dE| above 100 ulps of logp)."""
    if post:
        monkeypatch.setenv('MILE_TUNE_POST', '1')
    ospec = oracle.ModelSpec(5, (16, 16, 2))
    E, d, N = 3, ospec.n_params, 150
    prob = oracle.synthetic_problem(ospec, N, E, seed=21)
    rng = np.random.default_rng(7)
    t1, t2 = 48, 18
    extra = t2 // 3 if diag else 0
    z0 = rng.standard_normal((E, d)).astype(np.float32)
    noise = rng.standard_normal((t1 + t2 + extra, 2, E, d)).astype(np.float32)
    f32 = np.float32
    X, y = prob['X'].astype(f32), prob['y'].astype(f32)
    f = lambda th: oracle.logpost_and_grad(ospec, th, X, y)
    v0, v1, trust, n_eff = (5e-3, 1e-3, 1.5, 100) if diag else (0.5, 0.1, 1.5, 100)
    decay = f32((n_eff - 1.0) / (n_eff + 1.0))
    total = t1 + t2 + 1
    eng = _engine(ospec, prob['X'], prob['y'])
    st = oracle.mclmc_init(f, prob['theta0'].astype(f32), z0)
    L = np.full(E, max(math.sqrt(d), 15.0), f32)
    eps = np.full(E, 0.01, f32)
    sdc = np.ones((E, d), f32)
    kw = dict(desired_energy_var_start=v0, desired_energy_var_end=v1, trust_in_estimate=trust, decay_rate=float(decay))
    resolved = 0
    n_checked = 0

    def one_phase(st, eps, masks, noise_off, sdc_dev):
        nonlocal resolved, n_checked
        ad = oracle.AdaptiveState.fresh(E, d, f32)
        n_mask = sum(1 for m in masks if m == 1.0)
        for i, mask in enumerate(masks):
            z = noise[noise_off + i]
            # --- device: one step from the oracle's current (state, eps, adaptive state)
            dst = _to_dev_state(st)
            tuner = {k: torch.from_numpy(np.ascontiguousarray(v, f32)).cuda() for k, v in
                     dict(step_size=eps, step_size_max=ad.step_size_max, time=ad.time, x_average=ad.x_average,
                          stream_weight=ad.W, stream_average=ad.avg).items()}
            info_d = eng.tune(dst, tuner, torch.from_numpy(L), 1, schedule_step0=i, n_mask_steps=n_mask, schedule_total=total,
                              noise=torch.from_numpy(z[None]), sqrt_diag_cov=sdc_dev, want_info=True, **kw)
            torch.cuda.synchronize()
            # --- oracle: the same step in float32
            ad_in = ad.copy()
            var = oracle.desired_energy_var(i, total, v0, v1)
            st_n, eps_n, ok, info = oracle.tuner_step(f, st, eps, L, sdc, z[0], z[1], ad, mask=mask, var=var,
                                                      trust_in_estimate=trust, decay=decay)
            assert ok.all()
            where = f'phase offset {noise_off} step {i}'
            assert _rel(dst.position.cpu(), st_n.position) < 2e-5, where
            assert np.abs(dst.momentum.cpu().numpy() - st_n.momentum).max() < 2e-5, where
            assert _rel(dst.logdensity.cpu(), st_n.logdensity) < 2e-6, where
            dE_d = info_d.energy_change[0].cpu().numpy()
            ulp = float(np.spacing(f32(np.abs(st_n.logdensity).max())))
            assert np.abs(dE_d - info.energy_change).max() <= 16 * ulp + 1e-4 * np.abs(info.energy_change).max(), where
            # predictor on the device's own energy change, in the reference's arithmetic (float32)
            chk = ad_in.copy()
            chk.step_size_max = np.nan_to_num(chk.step_size_max)                     # accepted: nan_to_num(inf) = FLT_MAX
            eps_chk, _, _ = oracle.predictor_update(dE_d.astype(f32), eps, chk, dim=d, var=var, trust_in_estimate=trust, decay=decay)
            assert _rel(tuner['step_size'].cpu(), eps_chk) < 2e-5, where
            assert _rel(tuner['x_average'].cpu(), chk.x_average) < 2e-5 and _rel(tuner['time'].cpu(), chk.time) < 2e-5, where
            assert np.array_equal(tuner['step_size_max'].cpu().numpy(), chk.step_size_max), where
            if mask == 0.0:
                # the weight of this sample is the device's own new step size (checked above to 2e-5)
                assert _rel(tuner['stream_weight'].cpu(), ad_in.W + tuner['step_size'].cpu().numpy()) < 2e-5, where
                assert _rel(tuner['stream_average'].cpu(), ad.avg) < 2e-5 + 2 * _rel(tuner['step_size'].cpu(), eps_n), where
            else:
                assert np.array_equal(tuner['stream_weight'].cpu().numpy(), ad_in.W), where
            good = np.abs(info.energy_change) > 100 * ulp
            n_checked += E
            resolved += int(good.sum())
            if good.any():
                assert np.abs(tuner['step_size'].cpu().numpy() - eps_n)[good].max() / eps_n[good].max() < 1e-3, where
            st, eps = st_n, eps_n
        return st, eps, ad

    st, eps, ad = one_phase(st, eps, [1.0] * t1 + [0.0] * t2, 0, None)
    var_x = ad.avg[:, 1] - np.square(ad.avg[:, 0])
    assert np.all(var_x.sum(axis=1) > 0)
    if diag:
        assert d > 225 or True
        sdc = np.sqrt(np.maximum(var_x, 1e-12)).astype(f32)        # the clamp only guards the oracle-side sqrt of a rounding-negative
        st, eps, _ = one_phase(st, eps, [1.0] * extra, t1 + t2, torch.from_numpy(sdc))
    assert resolved >= 0.5 * n_checked, (resolved, n_checked)       # most steps have a resolved energy change
    assert np.all(np.isfinite(eps)) and np.all(eps > 0)


def test_phase3_at_a_realistic_horizon_matches_oracle(oracle):
    """make_adaptation_L (warmup.py:408-465) over 400 kept steps at a fixed step size (the regime of phase 3: no adaptive
    feedback, so fp32 and fp64 trajectories stay together -- oracle f32 vs f64: 5e-7 in L): the device's L -- 400 mile_step
    steps with every position kept, FFT / Geyer ESS in torch on the device -- against oracle.tune_phase3 in float64."""
    from mile_amd.warmup import mclmc_find_L_and_step_size
    ospec = oracle.ModelSpec(5, (8, 8, 2))
    E, d, t3 = 3, ospec.n_params, 400
    prob = oracle.synthetic_problem(ospec, 60, E, seed=21)
    rng = np.random.default_rng(5)
    z0 = rng.standard_normal((E, d)).astype(np.float32)
    nz = rng.standard_normal((t3, 2, E, d)).astype(np.float32)
    f = lambda th: oracle.logpost_and_grad(ospec, th, prob['X'], prob['y'])
    st = oracle.mclmc_init(f, prob['theta0'].astype(np.float64), z0.astype(np.float64))
    eps = np.full(E, 0.05)
    L0 = np.full(E, max(math.sqrt(d), 15.0))
    st3, L3 = oracle.tune_phase3(f, st, eps, L0, lambda i: (nz[i, 0].astype(np.float64), nz[i, 1].astype(np.float64)), t3)
    eng = _engine(ospec, prob['X'], prob['y'])
    s0 = eng.init(torch.from_numpy(prob['theta0']), noise=torch.from_numpy(z0))
    nd = torch.from_numpy(nz).cuda()
    state, params = mclmc_find_L_and_step_size(
        eng, s0, 0, tune1_steps=0, tune2_steps=0, tune3_steps=t3, step_size_init=0.05, desired_energy_var_start=0.5,
        desired_energy_var_end=0.1, trust_in_estimate=1.5, num_effective_samples=100, diagonal_preconditioning=False,
        noise_fn=lambda i: nd[i - 10 ** 9])
    assert torch.all(params.step_size == 0.05)
    assert _rel(params.L.cpu(), L3) < 1e-3
    assert _rel(state.position.cpu(), st3.position) < 1e-3
    assert np.all(L3 > 0.5) and np.all(L3 < 15.0)                   # the estimate moved off the phase-1 value


def test_dead_chain_fixture_device_equals_fp32_oracle_step_for_step(oracle):
    """the state that kills chains under the reference's stock tuner targets, driven on the device.
    tests/golden/dead_chain_b2.npz = one chain of the recorded airfoil run (profiles/r03/01_*), one step before it is thrown
    into a region with log-density -7e8 / |grad| 1.6e12.  From there, on the recorded Philox streams:
      * free-running, mile_tune reproduces its own record (same kernels, E = 1 instead of 128) and ends with
        x_average = inf, step_size = 0 -- every position, momentum and gradient finite, nothing ever rejected;
      * teacher-forced on the oracle's float32 run (tests/test_oracle.py::test_dead_chain_fixture_...), every step agrees
        with oracle.tuner_step: log-density and kinetic change 5e-3 (the bad region has sigma_min ~ 3e-4 and everything goes
        with 1 / sigma^2; E = 1 here splits the rows differently from the recorded E = 128 run: 2.3e-3 measured), the predictor on the device's own energy change 2e-5 -- through the overflow: xi / eps^6 = inf,
        x_average = inf, step_size = 0 exactly where the float32 formula says so."""
    import json
    fx = dict(np.load(GOLD / 'dead_chain_b2.npz', allow_pickle=False))
    dev = json.loads(str(fx['device_rows']))
    ospec = oracle.ModelSpec(5, tuple(int(v) for v in fx['hidden']))
    d = ospec.n_params
    tune1, tune2, total = (int(v) for v in fx['schedule'])
    v0, v1, trust, decay = (float(v) for v in fx['targets'])
    seed, step0, chain = int(fx['seed']), int(fx['step0']), int(fx['chain'])
    ids = torch.tensor([chain], dtype=torch.int32)
    eng = _engine(ospec, fx['X'], fx['y'])
    assert eng.grad_kernel == 'mfma_w64_bf16x3'
    f32 = np.float32
    kw = dict(n_mask_steps=tune1, schedule_total=total, desired_energy_var_start=v0, desired_energy_var_end=v1,
              trust_in_estimate=trust, decay_rate=decay, seed=seed, particle_ids=ids)
    Lt = torch.tensor([float(fx['L'])])

    def dev_tuner(eps, emax, time, xavg):
        mk = lambda v: torch.tensor([v], dtype=torch.float32, device='cuda')
        return {'step_size': mk(eps), 'step_size_max': mk(emax), 'time': mk(time), 'x_average': mk(xavg),
                'stream_weight': torch.zeros(1, device='cuda'), 'stream_average': torch.zeros((1, 2, d), device='cuda')}

    # ---- free-running on the device: its own record, then dead by overflow.  The chain is replicated to the 128 particles of
    # the recorded run (same chain id -> same noise) so that the grad kernel splits the rows as it did there: bit-identical sums.
    E0 = 128
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (E0,) + a.shape[1:]))
    st0 = oracle.State(fx['x'][None], fx['u'][None], np.array([fx['logp']], f32), fx['g'][None])
    dst = _to_dev_state(oracle.State(rep(st0.position), rep(st0.momentum), rep(st0.logdensity), rep(st0.logdensity_grad)))
    tuner = {k: v.expand(E0, *v.shape[1:]).contiguous() for k, v in dev_tuner(*(float(v) for v in fx['tuner'])).items()}
    kw_rep = dict(kw, particle_ids=ids.expand(E0).contiguous())
    n = len(dev)
    for i in range(n):
        info = eng.tune(dst, tuner, Lt.expand(E0).contiguous(), 1, schedule_step0=step0 + i, step_offset=step0 + i, want_info=True, **kw_rep)
        torch.cuda.synchronize()
        r = dev[i]
        assert torch.isfinite(dst.position).all() and torch.isfinite(dst.momentum).all() and torch.isfinite(dst.logdensity_grad).all()
        assert abs(info.logdensity[0, 0].item() - r['logdensity']) <= 1e-5 * abs(r['logdensity']), i
        assert abs(tuner['step_size'][0].item() - r['eps_out']) <= 1e-5 * r['eps_out'], i
        assert tuner['step_size_max'][0].item() > 3e38                                  # never rejected
        assert torch.equal(dst.position[0], dst.position[E0 - 1])                       # replicas stay identical
    dead_at = next(i for i, r in enumerate(dev) if r['eps_out'] == 0.0)
    assert 4 <= dead_at <= 10 and tuner['step_size'][0].item() == 0.0 and math.isinf(tuner['x_average'][0].item())
    assert dev[1]['energy_change'] > 1e10 and dev[1]['sigma_min'] < 1e-3 and dev[1]['rows_clipped'] == 0   # not the sigma clip

    # ---- teacher-forced on the oracle's float32 run
    X, y = fx['X'].astype(f32), fx['y'].astype(f32)
    f = lambda th: oracle.logpost_and_grad(ospec, th, X, y)
    st = st0
    ad = oracle.AdaptiveState(np.array([fx['tuner'][2]], f32), np.array([fx['tuner'][3]], f32), np.array([fx['tuner'][1]], f32),
                              np.zeros(1, f32), np.zeros((1, 2, d), f32))
    eps = np.array([fx['tuner'][0]], f32)
    L = np.array([fx['L']], f32)
    idn = np.array([chain])
    saw_overflow = False
    for i in range(14):
        k = step0 + i
        dst = _to_dev_state(st)
        tuner = dev_tuner(float(eps[0]), float(ad.step_size_max[0]), float(ad.time[0]), float(ad.x_average[0]))
        info_d = eng.tune(dst, tuner, Lt, 1, schedule_step0=k, step_offset=k, want_info=True, **kw)
        torch.cuda.synchronize()
        ad_in = ad.copy()
        eps_in = eps.copy()
        z1 = oracle.philox_normal(seed, idn, k, 0, d, dtype=np.float32)
        z2 = oracle.philox_normal(seed, idn, k, 1, d, dtype=np.float32)
        var = oracle.desired_energy_var(k, total, v0, v1)
        st, eps, ok, info = oracle.tuner_step(f, st, eps, L, np.ones((1, d), f32), z1, z2, ad, mask=1.0 if k < tune1 else 0.0,
                                              var=var, trust_in_estimate=trust, decay=f32(decay))
        assert ok[0]
        if eps_in[0] == 0.0:
            # a dead chain: eps = 0 moves nothing, dE = 0, and the formula keeps x_average = inf, step_size = 0
            assert torch.equal(dst.position.cpu(), torch.from_numpy(st.position)) and tuner['step_size'].item() == 0.0
            continue
        assert _rel(dst.position.cpu(), st.position) < 2e-5, i
        lp_d, lp_o = info_d.logdensity[0, 0].item(), float(info.logdensity[0])
        assert abs(lp_d - lp_o) <= 5e-3 * abs(lp_o), (i, lp_d, lp_o)
        dk_d, dk_o = info_d.kinetic_change[0, 0].item(), float(info.kinetic_change[0])
        assert abs(dk_d - dk_o) <= 5e-3 * abs(dk_o) + 1e-3, (i, dk_d, dk_o)
        # energy change: a difference of log-density-sized float32 numbers -- within 2e-3 of the LARGER of the two scales
        dE_d, dE_o = info_d.energy_change[0, 0].item(), float(info.energy_change[0])
        assert abs(dE_d - dE_o) <= 5e-3 * max(abs(lp_o), abs(dk_o)) + 1e-3, (i, dE_d, dE_o)
        chk = ad_in.copy()
        chk.step_size_max = np.nan_to_num(chk.step_size_max)
        eps_chk, _, _ = oracle.predictor_update(np.array([dE_d], f32), eps_in, chk, dim=d, var=var, trust_in_estimate=trust, decay=f32(decay))
        xa_d, xa_c = tuner['x_average'].item(), float(chk.x_average[0])
        if math.isinf(xa_c):
            saw_overflow = True
            assert math.isinf(xa_d) and tuner['step_size'].item() == 0.0 and eps_chk[0] == 0.0
        else:
            assert abs(xa_d - xa_c) <= 1e-4 * xa_c and abs(tuner['step_size'].item() - eps_chk[0]) <= 2e-5 * eps_chk[0], i
    assert eps[0] == 0.0 and math.isinf(float(ad.x_average[0]))          # the float32 oracle died as well


def test_device_tuner_matches_host_loop(oracle):
    """mile_tune (phases 1+2 on the device) == the host-driven loop over mile_step with the same noise."""
    from mile_amd.warmup import mclmc_find_L_and_step_size
    ospec = oracle.ModelSpec(5, (64, 64, 64, 2))
    E, d = 4, ospec.n_params
    prob = oracle.synthetic_problem(ospec, 100, E, seed=5)
    rng = np.random.default_rng(3)
    t1, t2 = 9, 4
    z0 = torch.from_numpy(rng.standard_normal((E, d)).astype(np.float32))
    n12 = torch.from_numpy(rng.standard_normal((t1 + t2, 2, E, d)).astype(np.float32)).cuda()
    eng = _engine(ospec, prob['X'], prob['y'])
    kw = dict(tune1_steps=t1, tune2_steps=t2, tune3_steps=0, step_size_init=0.002, desired_energy_var_start=0.5,
              desired_energy_var_end=0.1, trust_in_estimate=1.5, num_effective_samples=100,
              diagonal_preconditioning=False, noise_fn=lambda i: n12[i])
    out = {}
    for host in (True, False):
        s0 = eng.init(torch.from_numpy(prob['theta0']), noise=z0)
        out[host] = mclmc_find_L_and_step_size(eng, s0, 0, force_host_loop=host, **kw)
    (sh, ph), (sd, pd) = out[True], out[False]
    assert _rel(pd.step_size.cpu(), ph.step_size.cpu()) < 2e-3
    assert _rel(pd.L.cpu(), ph.L.cpu()) < 2e-3
    assert _rel(sd.position.cpu(), sh.position.cpu()) < 1e-3
    assert _rel(sd.logdensity.cpu(), sh.logdensity.cpu()) < 1e-4
    # diagonal preconditioning branch: sqrt_diag_cov from the tune2 variances, L = sqrt(d), extra steps
    kw['diagonal_preconditioning'] = True
    kw['step_size_init'] = 0.05
    n_extra = torch.from_numpy(rng.standard_normal((t1 + t2 + t2 // 3, 2, E, d)).astype(np.float32)).cuda()
    kw['noise_fn'] = lambda i: n_extra[i]
    outp = {}
    for host in (True, False):
        s0 = eng.init(torch.from_numpy(prob['theta0']), noise=z0)
        outp[host] = mclmc_find_L_and_step_size(eng, s0, 0, force_host_loop=host, **kw)
    # Var = E[x^2] - E[x]^2 in fp32 over a handful of barely-moved samples can cancel to <= 0 (NaN after sqrt)
    # in the reference arithmetic too: compare where both are finite and well above the cancellation floor
    a, b = outp[False][1].sqrt_diag_cov.cpu().numpy(), outp[True][1].sqrt_diag_cov.cpu().numpy()
    good = np.isfinite(a) & np.isfinite(b) & (b > 5e-3)
    assert good.mean() > 0.5 and np.abs(a[good] - b[good]).max() / b[good].max() < 2e-2
    assert torch.allclose(outp[False][1].L.cpu(), torch.full((E,), math.sqrt(d)))
    # one re-adjustment step with a ~1e-2 preconditioner moves eps by four orders of magnitude: 5 %
    assert _rel(outp[False][1].step_size.cpu(), outp[True][1].step_size.cpu()) < 5e-2


@pytest.mark.parametrize('F,hs,sdc,force_restart', [(5, (64, 64, 64, 2), False, False), (5, (16, 16, 2), False, False),
                                                    (7, (9, 6, 2), True, False), (5, (64, 64, 64, 2), False, True),
                                                    (7, (9, 6, 2), True, True)])
def test_merged_warmup_launch_matches_the_five_launch_form(oracle, monkeypatch, F, hs, sdc, force_restart):
    """Round 3: a warm-up step is four launches like a sampling step -- the record-point launch (B, O, record, tuner) also
    runs the NEXT step's O, B, A with the step size it has just computed, and writes them into the other ping-pong buffer.
    Against the five-launch form of rounds 1-2 (MILE_TUNE_NO_MERGE=1; also what a 1-step call does), same Philox streams,
    14 steps across the tune1 / tune2 boundary: same state, step sizes, adaptive state and streaming averages to fp32
    summation order.  Chain 1 starts at 1e18 (NaN gradient -> every step rejected): the merged launch then restarts the
    next step from the restored state inside the same kernel (upd_tune_restart) -- bit-identical bookkeeping expected.
    `force_restart`: the test hook MILE_TUNE_FORCE_RESTART sends EVERY chain through that restart path (what an accepted state
    that nan_to_num changed would take), which must give the same run."""
    if force_restart:
        monkeypatch.setenv('MILE_TUNE_FORCE_RESTART', '1')
    ospec = oracle.ModelSpec(F, hs)
    E, d = 4, ospec.n_params
    prob = oracle.synthetic_problem(ospec, 120, E, seed=9)
    th = prob['theta0'].copy()
    th[1] = 1e18
    eng = _engine(ospec, prob['X'], prob['y'])
    f32 = dict(dtype=torch.float32, device='cuda')
    rng = np.random.default_rng(4)
    sd = torch.from_numpy((0.5 + rng.random((E, d))).astype(np.float32)) if sdc else None
    n, t1 = 14, 8
    out = {}
    for merged in (True, False):
        if not merged:
            monkeypatch.setenv('MILE_TUNE_NO_MERGE', '1')
        st = eng.init(torch.from_numpy(th), seed=3)
        tuner = {'step_size': torch.full((E,), 2e-3, **f32), 'step_size_max': torch.full((E,), float('inf'), **f32),
                 'time': torch.zeros(E, **f32), 'x_average': torch.zeros(E, **f32),
                 'stream_weight': torch.zeros(E, **f32), 'stream_average': torch.zeros((E, 2, d), **f32)}
        info = eng.tune(st, tuner, torch.full((E,), 20.0), n, schedule_step0=0, n_mask_steps=t1, schedule_total=n + 1,
                        desired_energy_var_start=0.5, desired_energy_var_end=0.1, trust_in_estimate=1.5, decay_rate=99 / 101,
                        seed=7, step_offset=5, want_info=True, sqrt_diag_cov=sd)
        torch.cuda.synchronize()
        out[merged] = (st, {k: v.clone() for k, v in tuner.items()}, info)
    (sa, ta, ia), (sb, tb, ib) = out[True], out[False]
    live = [0, 2, 3]
    assert torch.equal(sa.position[1], sb.position[1]) and torch.equal(sa.position[1].cpu(), torch.from_numpy(th[1]))
    assert torch.equal(ta['step_size_max'][1], tb['step_size_max'][1]) and torch.equal(ta['step_size'][1], tb['step_size'][1])
    assert ta['step_size'][1].item() == pytest.approx(2e-3 * 0.8 ** n, rel=1e-5)
    assert ta['stream_weight'][1].item() == 0.0
    assert _rel(sa.position[live].cpu(), sb.position[live].cpu()) < 1e-4
    assert np.abs(sa.momentum[live].cpu().numpy() - sb.momentum[live].cpu().numpy()).max() < 1e-3
    assert _rel(sa.logdensity[live].cpu(), sb.logdensity[live].cpu()) < 1e-5
    assert _rel(sa.logdensity_grad[live].cpu(), sb.logdensity_grad[live].cpu()) < 1e-3
    # the predictor's weight exp(-(ln xi / 9)^2 / 2) turns rounding-level differences of a tiny energy change (the two forms
    # sum the same dot products in a different order) into 1e-3-sized differences of `time` on the d = 146 net (2.5e-3 measured)
    assert _rel(ta['step_size'][live].cpu(), tb['step_size'][live].cpu()) < 5e-3
    assert _rel(ta['x_average'][live].cpu(), tb['x_average'][live].cpu()) < 2e-2
    assert _rel(ta['time'][live].cpu(), tb['time'][live].cpu()) < 1e-2
    assert _rel(ta['stream_weight'][live].cpu(), tb['stream_weight'][live].cpu()) < 5e-3
    assert _rel(ta['stream_average'][live].cpu(), tb['stream_average'][live].cpu()) < 1e-3
    assert (sa.momentum[live].double().norm(dim=1) - 1).abs().max().item() < 1e-5
    assert ta['stream_weight'][0].item() > 0.0 and torch.isfinite(ia.energy_change[:, live]).all()


@pytest.mark.parametrize('F,hs,force_post', [(5, (64, 64, 64, 2), True), (9, (128, 128, 2), False)])
def test_device_tuner_post_kernel_matches_host_loop(oracle, monkeypatch, F, hs, force_post):
    """mile_tune's second form -- an ordinary kernel step plus k_tune_post -- which every net with d > 16384 takes
    (and a small one here through the MILE_TUNE_POST test hook), against the host-driven loop with the same noise."""
    from mile_amd.warmup import mclmc_find_L_and_step_size
    if force_post:
        monkeypatch.setenv('MILE_TUNE_POST', '1')
    ospec = oracle.ModelSpec(F, hs)
    E, d = 3, ospec.n_params
    assert force_post or d > 16384
    prob = oracle.synthetic_problem(ospec, 90, E, seed=6)
    rng = np.random.default_rng(8)
    t1, t2 = 7, 4
    z0 = torch.from_numpy(rng.standard_normal((E, d)).astype(np.float32))
    n12 = torch.from_numpy(rng.standard_normal((t1 + t2, 2, E, d)).astype(np.float32)).cuda()
    eng = _engine(ospec, prob['X'], prob['y'])
    assert eng.supports_device_tuner
    kw = dict(tune1_steps=t1, tune2_steps=t2, tune3_steps=0, step_size_init=0.002, desired_energy_var_start=0.5,
              desired_energy_var_end=0.1, trust_in_estimate=1.5, num_effective_samples=100,
              diagonal_preconditioning=False, noise_fn=lambda i: n12[i])
    out = {}
    for host in (True, False):
        s0 = eng.init(torch.from_numpy(prob['theta0']), noise=z0)
        out[host] = mclmc_find_L_and_step_size(eng, s0, 0, force_host_loop=host, **kw)
    (sh, ph), (sd, pd) = out[True], out[False]
    assert _rel(pd.step_size.cpu(), ph.step_size.cpu()) < 2e-3
    assert _rel(pd.L.cpu(), ph.L.cpu()) < 2e-3
    assert _rel(sd.position.cpu(), sh.position.cpu()) < 1e-3
    assert _rel(sd.logdensity.cpu(), sh.logdensity.cpu()) < 1e-4


@pytest.mark.parametrize('post', [False, True])
def test_device_tuner_rejects_nonfinite_steps(oracle, monkeypatch, post):
    """handle_nans on the device: a chain whose step leaves the finite numbers keeps its state and gets
    step_size_max = 0.8 eps; the other chains follow the predictor formula.  Both forms of mile_tune: the tuner
    fused into the record-point kernel, and the separate k_tune_post launch large nets take."""
    from mile_amd.warmup import predictor_update
    if post:
        monkeypatch.setenv('MILE_TUNE_POST', '1')
    ospec = oracle.ModelSpec(5, (16, 16, 2))
    E, d = 3, ospec.n_params
    prob = oracle.synthetic_problem(ospec, 80, E, seed=6)
    th = prob['theta0'].copy()
    th[1] = 1e18                                              # chain 1: the forward pass overflows -> NaN gradient
    eng = _engine(ospec, prob['X'], prob['y'])
    s0 = eng.init(torch.from_numpy(th), seed=1)
    st = type(s0)(*(t.clone() for t in s0))
    f32 = dict(dtype=torch.float32, device='cuda')
    eps0 = torch.full((E,), 1e-3, **f32)
    tuner = {'step_size': eps0.clone(), 'step_size_max': torch.full((E,), float('inf'), **f32),
             'time': torch.zeros(E, **f32), 'x_average': torch.zeros(E, **f32),
             'stream_weight': torch.zeros(E, **f32), 'stream_average': torch.zeros((E, 2, d), **f32)}
    info = eng.tune(st, tuner, torch.full((E,), 20.0), 1, schedule_step0=0, n_mask_steps=0, schedule_total=10,
                    desired_energy_var_start=0.5, desired_energy_var_end=0.1, trust_in_estimate=1.5,
                    decay_rate=99 / 101, seed=1, want_info=True)
    torch.cuda.synchronize()
    assert torch.equal(st.position[1], s0.position[1])                       # reverted
    assert not torch.equal(st.position[0], s0.position[0]) and torch.isfinite(st.position[[0, 2]]).all()
    assert tuner['step_size_max'][1].item() == pytest.approx(0.8e-3, rel=1e-6)
    assert tuner['step_size_max'][0].item() > 3e38                            # nan_to_num(inf)
    assert tuner['stream_weight'][1].item() == 0.0 and tuner['stream_weight'][0].item() > 0.0
    dE = info.energy_change[0].clone()
    dE[1] = 0.0                                                               # rejected: energy change 0.0
    ref, _, _ = predictor_update(dE, eps0, torch.zeros(E, **f32), torch.zeros(E, **f32), tuner['step_size_max'],
                                 dim=d, desired_var=0.5, trust_in_estimate=1.5, decay_rate=99 / 101)
    assert _rel(tuner['step_size'].cpu(), ref.cpu()) < 1e-4
    assert tuner['step_size'][1].item() == pytest.approx(0.8e-3, rel=1e-5)    # clipped at step_size_max
    # streaming average after one accepted tune2 step is the position itself
    assert torch.allclose(tuner['stream_average'][0, 0], st.position[0])
    assert torch.allclose(tuner['stream_average'][0, 1], st.position[0] ** 2)


def test_inference_loop_writes_reference_layout(oracle, tmp_path):
    from mile_amd.callbacks import load_samples_from_dir
    from mile_amd.config import SamplerConfig
    from mile_amd.probabilistic import ProbabilisticModel
    from mile_amd.sampling import inference_loop, kept_indices
    from mile_amd.tree import PRNGKey
    ospec = oracle.ModelSpec(5, (16, 16, 2))
    prob = oracle.synthetic_problem(ospec, 150, 4, seed=8)
    pm = ProbabilisticModel(_spec(ospec), task='regr')
    cfg = SamplerConfig(name='mclmc', warmup_steps=60, n_chains=4, n_samples=45, n_thinning=10,
                        desired_energy_var_start=0.5, desired_energy_var_end=0.1, step_size_init=0.001)
    step_ids = np.array([4, 5, 6, 7])
    kept = inference_loop(pm.bind(torch.from_numpy(prob['X']), torch.from_numpy(prob['y'])), cfg, PRNGKey(4),
                          torch.from_numpy(prob['theta0']), step_ids, tmp_path / 'samples', return_samples=True,
                          chunk_steps=20)
    idx = kept_indices(45, 10).tolist()
    assert idx == [0, 10, 20, 30, 40]
    for c in step_ids:                                              # integer file naming is exact
        assert sorted(p.name for p in (tmp_path / 'samples' / str(c)).iterdir()) == sorted(f'sample_{n}.npz' for n in idx)
    assert (tmp_path / 'samples' / 'info.pkl').exists()
    lines = (tmp_path / 'warmup_params.txt').read_text().strip().split('\n')
    assert len(lines) == 2 and all(len(l.split(',')) == 4 for l in lines)
    eps = np.array([float(v) for v in lines[0].split(',')])
    assert np.all(eps > 0) and np.all(np.isfinite(eps))
    back = load_samples_from_dir(tmp_path / 'samples', pm.spec)     # [chains, saved, d]
    assert back.shape == (4, 5, ospec.n_params)
    assert np.array_equal(back, kept.permute(1, 0, 2).numpy())      # files hold exactly the kept positions
    assert np.isfinite(back).all()


@pytest.mark.parametrize('n_chains,n_thinning,chunk_steps', [(1, 2, 8), (3, 8, 8), (1, 8, 8)])
def test_sample_files_do_not_alias_the_pinned_buffers(oracle, tmp_path, n_chains, n_thinning, chunk_steps):
    """with ONE chain per rank, or ONE kept sample per chunk, a chain's slice of the pinned D2H
    buffer is already contiguous; handing the view to the writer pool let a later chunk's copy overwrite it before the
    feeder thread pickled it.  >= 5 chunks through the two pinned slots; every file must hold its own chunk's draw."""
    from mile_amd.callbacks import load_samples_from_dir
    from mile_amd.config import SamplerConfig
    from mile_amd.probabilistic import ProbabilisticModel
    from mile_amd.sampling import inference_loop
    from mile_amd.tree import PRNGKey
    ospec = oracle.ModelSpec(5, (16, 16, 2))
    prob = oracle.synthetic_problem(ospec, 150, n_chains, seed=9)
    pm = ProbabilisticModel(_spec(ospec), task='regr')
    cfg = SamplerConfig(name='mclmc', warmup_steps=40, n_chains=n_chains, n_samples=48, n_thinning=n_thinning,
                        desired_energy_var_start=5e-4, desired_energy_var_end=1e-4, step_size_init=0.001)
    kept = inference_loop(pm.bind(torch.from_numpy(prob['X']), torch.from_numpy(prob['y'])), cfg, PRNGKey(2),
                          torch.from_numpy(prob['theta0']), np.arange(n_chains), tmp_path / 'samples',
                          return_samples=True, chunk_steps=chunk_steps, io_workers=2)
    back = load_samples_from_dir(tmp_path / 'samples', pm.spec)     # [chains, saved, d]
    assert back.shape == (n_chains, 48 // n_thinning, ospec.n_params)
    assert np.array_equal(back, kept.permute(1, 0, 2).numpy())
    assert len({back[0, s].tobytes() for s in range(back.shape[1])}) == back.shape[1]   # all draws distinct


def test_train_cli_runs_the_yaml_surface(tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=30, n_chains=4)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, str(ROOT / 'train.py'), '-c', str(tmp_path / 'cfg.yaml'), '-d', '1'],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp = tmp_path / 'smoke_synthetic'
    assert (exp / 'config.yaml').exists() and (exp / 'warmup_params.txt').exists() and (exp / 'tree').exists()
    assert sorted(p.name for p in (exp / 'samples').iterdir() if p.is_dir()) == ['0', '1', '2', '3']
    assert sorted(p.name for p in (exp / 'samples' / '2').iterdir()) == ['sample_0.npz', 'sample_10.npz', 'sample_20.npz']
    log = (exp / 'training.log').read_text()
    assert 'time.sampling took' in log and 'Starting mclmc Sampling' in log
    # evaluate.py: LPPD of the saved samples on the held-out split, through mile_pointwise_loglik
    r = subprocess.run([sys.executable, str(ROOT / 'evaluate.py'), '-e', str(exp)], capture_output=True, text=True, cwd=ROOT,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import json
    m = json.loads((exp / 'metrics.json').read_text())
    assert (m['n_chains'], m['n_samples'], m['split']) == (4, 3, 'test') and m['nonfinite_samples'] == 0
    assert np.isfinite(m['lppd']) and np.isfinite(m['nll_mean']) and m['lppd'] >= -m['nll_mean'] - 1e-6   # Jensen


def test_train_cli_with_warmstart_training(tmp_path):
    """`warmstart.include: true`: the deep-ensemble members are trained (reference optimizer / epoch / early-stopping
    schedule on full-batch engine gradients) and the chains start from them."""
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['experiment_name'] = 'ws'
    cfg['training']['warmstart'] = {'include': True, 'optimizer_config': {'name': 'adamw', 'parameters': {'learning_rate': 0.003, 'weight_decay': 0.001}},
                                    'max_epochs': 6, 'batch_size': 128, 'patience': 3}
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=20, n_chains=3, desired_energy_var_start=5e-4, desired_energy_var_end=1e-4)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, str(ROOT / 'train.py'), '-c', str(tmp_path / 'cfg.yaml'), '-d', '1'],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp = tmp_path / 'ws'
    log = (exp / 'training.log').read_text()
    assert 'Warmstart Training completed' in log and 'time.warmstart took' in log
    z = np.load(exp / 'warmstart' / 'params_2.npz')
    assert np.abs(z['fcn.layer0.bias']).max() > 0                 # module.init starts biases at zero: they were trained
    assert all(np.isfinite(z[k]).all() for k in z.files)
    assert sorted(p.name for p in (exp / 'samples' / '1').iterdir()) == ['sample_0.npz', 'sample_10.npz']


@pytest.mark.parametrize('F,hs,act,task,opt', [
    (5, (16, 16, 2), 'relu', 'regr', 'adamw'), (5, (64, 64, 64, 2), 'relu', 'regr', 'adam'),
    (11, (32, 7), 'sigmoid', 'classification', 'sgd'), (9, (128, 128, 2), 'relu', 'regr', 'adamw'),
])
def test_fused_warmstart_step_matches_the_optax_rules(oracle, monkeypatch, F, hs, act, task, opt):
    """mile_warmstart_step (round 3: likelihood gradient of the row window + ONE fused optimizer launch, in place) against the
    host-side restatement of optax's update rules (`warmstart._Optimizer`, CPU-tested) driven by the ORACLE's gradient of the
    batch-mean negative log-likelihood: six minibatch steps over three windows, one member frozen (early stopping) --
    parameters, moments and the reported batch NLL.  (The reference gradient must be the likelihood's own: forming it as
    `grad(log posterior) - grad(log prior)` leaves rounding residue on units whose likelihood gradient is exactly zero, and
    Adam's m / sqrt(v) turns any residue into a full-size update -- 1.6e-4 of max |theta| after six steps, measured.)"""
    from mile_amd.warmstart import _Optimizer
    ospec = oracle.ModelSpec(F, hs, activation=act, task=task)
    E, N, bs = 4, 96, 32
    prob = oracle.synthetic_problem(ospec, N, E, seed=17)
    eng = _engine(ospec, prob['X'], prob['y'])
    monkeypatch.setattr(oracle, 'log_prior', lambda spec, th: (np.zeros(th.shape[0], th.dtype), np.zeros_like(th)))
    params = {'learning_rate': 0.01, 'weight_decay': 0.001}
    th_a = torch.from_numpy(prob['theta0']).cuda().contiguous()
    th_b = torch.from_numpy(prob['theta0']).clone()
    ref = _Optimizer(opt, params, th_b)
    ost = {'name': opt, 'learning_rate': ref.lr, 'b1': ref.b1, 'b2': ref.b2, 'eps': ref.eps, 'weight_decay': ref.wd, 't': 0,
           'm': torch.zeros_like(th_a), 'v': torch.zeros_like(th_a)}
    active = torch.tensor([True, True, False, True])
    for k in range(6):
        r0 = (k % 3) * bs
        eng.set_row_window(r0, bs)
        nll_a = eng.warmstart_step(th_a, ost, active.cuda(), want_nll=True)
        ll, gl = oracle.logpost_and_grad(ospec, th_b.numpy().astype(np.float64), prob['X'][r0:r0 + bs], prob['y'][r0:r0 + bs])
        nll_b = -ll / bs
        th_b = ref.step(th_b, torch.from_numpy((-gl / bs).astype(np.float32)), active)
        assert _rel(nll_a[active.cuda()].cpu(), nll_b[active.numpy()]) < 1e-4, k
    eng.set_row_window(0, 0)
    torch.cuda.synchronize()
    assert torch.equal(th_a[2].cpu(), torch.from_numpy(prob['theta0'][2]))              # frozen member untouched
    # sgd: fp32 rounding of the gradient only.  adam / adamw divide by sqrt(v) + 1e-8: on entries whose likelihood gradient is
    # itself rounding-sized (|g| <~ 1e-7 max |g|: nearly-dead units) m / sqrt(v) is O(1) whatever the noise is, so fp32 and fp64
    # gradients give updates that differ by a good part of lr there -- up to 1.7e-4 of max |theta| after six steps (measured;
    # fp32 JAX against fp64 JAX would show the same).  The moments themselves agree to 1e-4.
    assert _rel(th_a.cpu(), th_b) < (2e-5 if opt == 'sgd' else 5e-4)
    if opt != 'sgd':
        assert _rel(ost['m'].cpu(), ref.m) < 1e-4 and _rel(ost['v'].cpu(), ref.v) < 1e-4
        assert ost['m'][2].abs().max().item() == 0.0 and ost['t'] == 6


def test_train_cli_classification_wide_net(tmp_path):
    """The YAML surface on a covertype-shaped problem (7 classes, wide hidden layers -> the layer-wise
    SGEMM path chosen by AUTO, the host-driven tuner because d > 16384)."""
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'mclmc_covertype_b4.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['experiment_name'] = 'b4_small'
    cfg['data']['path'] = '1500x54'
    cfg['model']['hidden_structure'] = [128, 128, 7]
    # phase 2 estimates L = sqrt(sum(E[x^2] - E[x]^2)) in fp32 as the reference does (warmup.py:204-228): with
    # prior-scale positions that difference only rises above rounding after a few dozen steps, hence 400 here
    cfg['training']['sampler'].update(warmup_steps=400, n_samples=20, n_chains=3, desired_energy_var_start=5e-4,
                                      desired_energy_var_end=1e-4)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, str(ROOT / 'train.py'), '-c', str(tmp_path / 'cfg.yaml'), '-d', '1'],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp = tmp_path / 'b4_small'
    assert sorted(p.name for p in (exp / 'samples').iterdir() if p.is_dir()) == ['0', '1', '2']
    z = np.load(exp / 'samples' / '1' / 'sample_10.npz')
    assert z['fcn.layer0.kernel'].shape == (54, 128) and z['fcn.layer2.bias'].shape == (7,)
    assert all(np.isfinite(z[k]).all() for k in z.files)


LPPD_GATE_CASES = [
    # in_features, hidden, activation, task, N, E, T, step-size factor, grad kernel the engine must resolve to
    # the reference's stock net shape on the kernel AUTO selects for it (round 3: k_grad_narrow), a sigmoid softmax net on the
    # same kernel, and a width only the generic kernel covers
    (5, (16, 16, 2), 'relu', 'regr', 200, 4, 60, 3.0, 'mfma_narrow_f32'),
    (54, (32, 7), 'sigmoid', 'classification', 400, 4, 60, 1.0, 'mfma_narrow_f32'),
    (5, (72, 72, 2), 'relu', 'regr', 200, 4, 60, 3.0, 'generic'),
    (5, (64, 64, 3), 'tanh', 'classification', 300, 4, 60, 1.0, 'mfma_narrow_f32'),     # widths 33..64: the LDS-weight form
    # BASELINE config B1 (airfoil shape, 3x64 MLP, 16 particles) on the kernel AUTO selects
    (5, (64, 64, 64, 2), 'relu', 'regr', 1052, 16, 120, 1.0, 'mfma_w64_bf16x3'),
    # the layer-wise MFMA GEMM path on a small softmax net (B4's head)
    (11, (96, 96, 5), 'relu', 'classification', 300, 6, 100, 1.0, 'mfma_wide_bf16x3'),
]


@pytest.mark.parametrize('F,hs,act,task,N,E,T,eps_mul,kernel', LPPD_GATE_CASES)
def test_lppd_matches_oracle_after_equal_step_count(oracle, F, hs, act, task, N, E, T, eps_mul, kernel):
    """The +-1 % LPPD gate of BASELINE.json: the device sampler and the fp64 oracle run the same number of steps from
    the same state on the SAME noise; the LPPD of their kept samples on held-out rows must agree within 1 %.
    Every production grad kernel family has a case: the narrow-net kernel (both heads), generic, the AUTO kernel at the B1
    shape, the GEMM path."""
    from mile_amd.metrics import lppd
    ospec = oracle.ModelSpec(F, hs, activation=act, task=task)
    thin, Nt = 5, 77
    full = oracle.synthetic_problem(ospec, N + Nt, E, seed=31)
    Xtr, ytr, Xt, yt = full['X'][:N], full['y'][:N], full['X'][N:], full['y'][N:]
    rng = np.random.default_rng(9)
    d = ospec.n_params
    z0 = rng.standard_normal((E, d)).astype(np.float32)
    noise = rng.standard_normal((T, 2, E, d)).astype(np.float32)
    f = lambda th: oracle.logpost_and_grad(ospec, th, Xtr, ytr)
    st = oracle.mclmc_init(f, full['theta0'].astype(np.float64), z0.astype(np.float64))
    st, okept, oidx = oracle.sample_chain(f, st, full['eps'].astype(np.float64) * eps_mul, full['L'].astype(np.float64),
                                          lambda i: (noise[i, 0].astype(np.float64), noise[i, 1].astype(np.float64)), T, thin)
    assert oidx.tolist() == list(range(0, T, thin))
    o_out = oracle.mlp_forward(ospec, okept.reshape(-1, d), Xt).reshape(len(oidx), E, Nt, hs[-1]).transpose(1, 0, 2, 3)
    o_lppd = oracle.lppd(oracle.pointwise_lppd(ospec, o_out, yt))
    eng = _engine(ospec, Xtr, ytr)                                        # grad_kernel = 'auto'
    assert eng.grad_kernel == kernel
    s = eng.init(torch.from_numpy(full['theta0']), noise=torch.from_numpy(z0))
    s, _, kept = eng.step(s, torch.from_numpy(full['eps']) * eps_mul, torch.from_numpy(full['L']), n_steps=T,
                          noise=torch.from_numpy(noise), n_thinning=thin)
    pw = eng.pointwise_loglik(kept.permute(1, 0, 2).contiguous(), torch.from_numpy(Xt), torch.from_numpy(yt))   # [C, S, Nt]
    got = lppd(pw).item()
    print(f'LPPD gate {kernel}: device {got:.6f} oracle {o_lppd:.6f} rel {abs(got - o_lppd) / abs(o_lppd):.2e}; '
          f'final position rel err {_rel(s.position.cpu(), st.position):.2e}')
    assert np.isfinite(got) and abs(got - o_lppd) < 0.01 * abs(o_lppd), (got, o_lppd)


def test_bf16_kernel_lppd_within_one_percent_of_fp32(oracle):
    """BASELINE config 3 runs with bf16 matrix operands: the +-1 % LPPD gate for that kernel, against the
    fp32 kernel (itself checked against the oracle above) after the same number of steps from the same
    state with the same noise.  Trajectories decorrelate under the 1e-2 gradient perturbation, so this is a
    statement about the sampled predictive, not a bitwise one."""
    from mile_amd.metrics import lppd, pointwise_lppd, predict
    ospec = oracle.ModelSpec(9, (128, 128, 128, 2))
    E, T, N = 32, 200, 600
    prob = oracle.synthetic_problem(ospec, N, E, seed=5)
    rng = np.random.default_rng(2)
    Xt = rng.standard_normal((150, 9)).astype(np.float32)
    yt = rng.standard_normal(150).astype(np.float32)
    got = {}
    for k in ('generic', 'mfma_w128_bf16'):
        eng = _engine(ospec, prob['X'], prob['y'], k)
        assert eng.grad_kernel == k
        s = eng.init(torch.from_numpy(prob['theta0']), seed=11)
        s, info, kept = eng.step(s, torch.from_numpy(prob['eps']), torch.from_numpy(prob['L']), n_steps=T, seed=12,
                                 n_thinning=5)
        assert torch.isfinite(s.position).all() and torch.isfinite(info.energy_change).all()
        out = predict(_spec(ospec), kept.permute(1, 0, 2), torch.from_numpy(Xt).cuda())
        got[k] = lppd(pointwise_lppd(out, torch.from_numpy(yt), 'regr')).item()
    assert abs(got['mfma_w128_bf16'] - got['generic']) < 0.01 * abs(got['generic']), got


@pytest.mark.parametrize('F,hs,act,task,kernels', [
    (5, (64, 64, 64, 2), 'relu', 'regr', ('mfma_w64', 'mfma_w64_bf16x3', 'generic')),
    (5, (64, 2), 'relu', 'regr', ('mfma_w64', 'generic')),
    (9, (24, 17, 2), 'tanh', 'regr', ('generic',)),
    (11, (32, 7), 'sigmoid', 'classification', ('generic', 'gemm_f32', 'mfma_wide_bf16x3')),
    # wide nets evaluate through the strided-batched SGEMM forward (fp32 also when sampling ran on bf16 operands)
    (9, (128, 128, 128, 2), 'relu', 'regr', ('gemm_f32', 'mfma_w128_bf16', 'mfma_wide_bf16x3')),
    (54, (256, 256, 7), 'tanh', 'classification', ('gemm_f32', 'auto')),
    (5, (16, 16, 2), 'relu', 'regr', ('mfma_narrow_f32',)),       # the narrow kernel's engines evaluate on k_fwd_generic
])
def test_pointwise_loglik_kernel_matches_oracle(oracle, F, hs, act, task, kernels):
    from mile_amd.metrics import lppd
    ospec = oracle.ModelSpec(F, hs, activation=act, task=task)
    C, S, N, Nt = 3, 5, 90, 301                     # 301 = the airfoil test split
    prob = oracle.synthetic_problem(ospec, N, C * S, seed=12)
    test = oracle.synthetic_problem(ospec, Nt, 1, seed=13)
    samples = prob['theta0'].reshape(C, S, -1)
    out = oracle.mlp_forward(ospec, prob['theta0'].astype(np.float64), test['X']).reshape(C, S, Nt, -1)
    ref = oracle.pointwise_lppd(ospec, out, test['y'])
    for k in kernels:
        eng = _engine(ospec, prob['X'], prob['y'], k)
        pw = eng.pointwise_loglik(torch.from_numpy(samples), torch.from_numpy(test['X']), torch.from_numpy(test['y']))
        assert pw.shape == (C, S, Nt)
        assert np.abs(pw.cpu().numpy() - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())
        assert abs(lppd(pw).item() - oracle.lppd(ref)) < 1e-4 * abs(oracle.lppd(ref))


def test_lppd_long_run_agrees_with_cpu_sampler_statistically(oracle):
    """BASELINE's +-1 % LPPD gate over a LONG run.  Two samplers that share start, step size and the Philox
    noise stream but not their rounding (HIP kernels vs the C/OpenMP restatement) decorrelate within a few
    hundred steps; their posterior predictive must still agree within Monte-Carlo error (128 chains x 290 kept samples)."""
    from mile_amd.metrics import lppd
    from oracle.cpu_c import CpuPort
    ospec = oracle.ModelSpec(5, (16, 16, 2))
    E, T, N, thin, burn = 128, 3000, 256, 10, 10
    full = oracle.synthetic_problem(ospec, N + 301, E, seed=41)
    Xtr, ytr, Xte, yte = full['X'][:N], full['y'][:N], full['X'][N:], full['y'][N:]
    d = ospec.n_params
    ids = np.arange(E)
    seed = 77
    eps = np.full(E, 0.05, np.float32)
    L = np.full(E, 2.0 * math.sqrt(d), np.float32)
    # CPU sampler (fp32 C port) fed with the same counter-RNG stream
    port = CpuPort(ospec, Xtr, ytr)
    x = full['theta0'].copy()
    z0 = oracle.philox_normal(seed, ids, 0, 2, d, dtype=np.float32)
    u = (z0 / np.linalg.norm(z0, axis=1, keepdims=True)).astype(np.float32)
    logp, g = port.logpost_grad(x)
    kept_c = []
    for i0 in range(0, T, thin):
        noise = np.stack([np.stack([oracle.philox_normal(seed, ids, i, 0, d, dtype=np.float32),
                                    oracle.philox_normal(seed, ids, i, 1, d, dtype=np.float32)]) for i in range(i0, i0 + thin)])
        # kept index i0 is the position after step i0: run one step, record, run the other thin-1
        port.steps(x, u, logp, g, eps, L, noise[:1])
        kept_c.append(x.copy())
        port.steps(x, u, logp, g, eps, L, noise[1:])
    first_c = kept_c[0]
    kept_c = np.stack(kept_c)[burn:]                                     # [K, E, d]
    o_out = oracle.mlp_forward(ospec, kept_c.reshape(-1, d).astype(np.float64), Xte).reshape(-1, E, 301, 2).transpose(1, 0, 2, 3)
    c_lppd = oracle.lppd(oracle.pointwise_lppd(ospec, o_out, yte))
    # HIP sampler
    eng = _engine(ospec, Xtr, ytr)
    tid = torch.from_numpy(ids.astype(np.int32))
    s = eng.init(torch.from_numpy(full['theta0']), seed=seed, particle_ids=tid)
    s, _, kept = eng.step(s, torch.from_numpy(eps), torch.from_numpy(L), n_steps=T, seed=seed, n_thinning=thin,
                          particle_ids=tid)
    assert kept.shape[0] == T // thin
    # the two samplers start identically: first kept sample agrees to fp32 rounding
    assert _rel(kept[0].cpu(), first_c) < 1e-4
    pw = eng.pointwise_loglik(kept[burn:].permute(1, 0, 2).contiguous(), torch.from_numpy(Xte), torch.from_numpy(yte))
    got = lppd(pw).item()
    # Two samplers whose trajectories have decorrelated are two Monte-Carlo estimates of the same LPPD: the bound is
    # statistical.  Standard error of the DIFFERENCE by a delete-one-group jackknife over 8 groups of 16 chains (both
    # samplers leave out the same chains); the gate is 3 SE, and the SE itself must be small enough (< 1 % of the LPPD)
    # for the gate to mean something.  Measured in round 1: -0.3210 (HIP) vs -0.3171 (CPU), 1.2 %.
    # On EQUAL noise the agreement is 1e-4 (test_lppd_matches_oracle_after_equal_step_count): that is the +-1 % gate.
    pw_c = oracle.pointwise_lppd(ospec, o_out, yte)                          # [C, S, N]
    pw_h = pw.cpu().numpy().astype(np.float64)
    G = 8
    diffs = []
    for gi in range(G):
        keep = np.ones(E, dtype=bool)
        keep[gi * (E // G):(gi + 1) * (E // G)] = False
        diffs.append(oracle.lppd(pw_h[keep]) - oracle.lppd(pw_c[keep]))
    diffs = np.asarray(diffs)
    se = math.sqrt((G - 1) / G * ((diffs - diffs.mean()) ** 2).sum())
    print(f'long-run LPPD: HIP {got:.4f}  CPU port {c_lppd:.4f}  diff {got - c_lppd:+.4f}  jackknife SE {se:.4f}')
    assert se < 0.01 * abs(c_lppd), se
    assert np.isfinite(got) and abs(got - c_lppd) < max(3.0 * se, 0.002 * abs(c_lppd)), (got, c_lppd, se)


def test_full_size_properties_b2(oracle):
    """Size-independent properties at BASELINE's full B2 size (N=1052, E=128, d=8834)."""
    ospec, N, E = oracle.config_spec('B2')
    prob = oracle.synthetic_problem(ospec, N, E, seed=0)
    # 128 particles x 1052 rows x 192 hidden units = 26 M pre-activations: 40 rows have one within fp32 rounding of the ReLU
    # kink (|z| < 3e-7 of the layer's largest), where two correct fp32 kernels may legitimately take different sides (the
    # three-term kernel sums its products in another order than the VALU kernel: 1.7e-4 of max |g| on such a row, measured).
    # Those rows are left out for every kernel alike, as in tests/test_gpu_parity.py.
    _, zs, _ = oracle.mlp_forward(ospec, prob['theta0'].astype(np.float64), prob['X'], keep=True)
    near = np.zeros(N, dtype=bool)
    for z in zs[:-1]:
        near |= (np.abs(z) < 3e-7 * np.abs(z).max()).any(axis=(0, 2))
    assert 0 < near.sum() <= 64, near.sum()
    prob = dict(prob, X=np.ascontiguousarray(prob['X'][~near]), y=np.ascontiguousarray(prob['y'][~near]))
    th = torch.from_numpy(prob['theta0'])
    mf = _engine(ospec, prob['X'], prob['y'], 'auto')          # the shipped / benched kernel
    assert mf.grad_kernel == 'mfma_w64_bf16x3'
    ge = _engine(ospec, prob['X'], prob['y'], 'generic')
    lp1, g1 = mf.logpost_grad(th)
    lp2, g2 = ge.logpost_grad(th)
    # two independent HIP implementations agree
    assert _rel(lp1.cpu(), lp2.cpu()) < 2e-6 and _rel(g1.cpu(), g2.cpu()) < 2e-5
    # a subset against the fp64 oracle
    lo, go = oracle.logpost_and_grad(ospec, prob['theta0'][:6].astype(np.float64), prob['X'], prob['y'])
    assert _rel(lp1[:6].cpu(), lo) < 2e-6 and _rel(g1[:6].cpu(), go) < 2e-5
    # additivity over data: likelihood gradient of all rows == sum over two halves (the prior counted once)
    h = 500
    a = _engine(ospec, prob['X'][:h], prob['y'][:h], 'auto').logpost_grad(th)
    b = _engine(ospec, prob['X'][h:], prob['y'][h:], 'auto').logpost_grad(th)
    prior_g = -th.cuda()
    assert _rel((a[1] + b[1] - prior_g).cpu(), g1.cpu()) < 2e-5
    prior_v = (-0.5 * th.double() ** 2).sum(1) - ospec.n_params * 0.5 * math.log(2 * math.pi)
    assert _rel((a[0].cpu().double() + b[0].cpu().double() - prior_v), lp1.cpu()) < 2e-6
    # steps: unit momentum, determinism, finite energy bookkeeping
    ids = torch.arange(E, dtype=torch.int32)
    s0 = mf.init(th, seed=5, particle_ids=ids)
    s1, info, kept = mf.step(s0, torch.from_numpy(prob['eps']), torch.from_numpy(prob['L']), n_steps=20, seed=5,
                             n_thinning=10, particle_ids=ids)
    s1b, info_b, _ = mf.step(s0, torch.from_numpy(prob['eps']), torch.from_numpy(prob['L']), n_steps=20, seed=5,
                             n_thinning=10, particle_ids=ids)
    assert torch.equal(s1.position, s1b.position) and torch.equal(info.energy_change, info_b.energy_change)
    assert (s1.momentum.double().norm(dim=1) - 1).abs().max().item() < 1e-5
    assert kept.shape == (2, E, ospec.n_params) and torch.isfinite(kept).all()
    assert torch.isfinite(info.energy_change).all()
    # energy_change = kinetic_change - l_new + l_old, consistently
    l_prev = torch.cat([s0.logdensity[None], info.logdensity[:-1]])
    assert (info.energy_change - (info.kinetic_change - info.logdensity + l_prev)).abs().max().item() < 5e-2


def test_full_size_properties_b3(oracle):
    """Size-independent properties at BASELINE's full B3 size (N=36000, E=512, d=34562) for the bf16-operand
    kernel: agreement with the fp32 layer-wise path, additivity over data, permutation equivariance over
    particles (bit-exact), determinism and unit momentum through steps."""
    ospec, N, E = oracle.config_spec('B3')
    prob = oracle.synthetic_problem(ospec, N, E, seed=0)
    th = torch.from_numpy(prob['theta0'])
    bf = _engine(ospec, prob['X'], prob['y'], 'mfma_w128_bf16')
    lp1, g1 = bf.logpost_grad(th)
    # against the fp32 layer-wise path (itself checked against the oracle at small sizes) on a slice of the particles
    ge = _engine(ospec, prob['X'], prob['y'], 'gemm_f32')
    lp2, g2 = ge.logpost_grad(th[:32])
    assert _rel(lp1[:32].cpu(), lp2.cpu()) < 5e-3
    rel = ((g1[:32] - g2).norm(dim=1) / g2.norm(dim=1)).max().item()
    assert rel < 5e-2, rel
    # a few particles against the oracle's bf16 recipe (fp64)
    lo, go = oracle.logpost_and_grad_bf16(ospec, prob['theta0'][:2].astype(np.float64), prob['X'], prob['y'])
    assert _rel(lp1[:2].cpu(), lo) < 1e-4
    assert ((g1[:2].cpu().double() - torch.from_numpy(go)).norm(dim=1) / torch.from_numpy(go).norm(dim=1)).max().item() < 5e-3
    # additivity over data (rows are rounded to bf16 one by one, so halves add up to fp32 summation order)
    h = 17984                                               # a multiple of 64: both halves keep their row tiles
    a = _engine(ospec, prob['X'][:h], prob['y'][:h], 'mfma_w128_bf16').logpost_grad(th)
    b = _engine(ospec, prob['X'][h:], prob['y'][h:], 'mfma_w128_bf16').logpost_grad(th)
    prior_g = -th.cuda()
    assert _rel((a[1] + b[1] - prior_g).cpu(), g1.cpu()) < 2e-5
    # particles are independent: a permutation of the rows of theta permutes the outputs bit for bit
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(1))
    lp3, g3 = bf.logpost_grad(th[perm])
    assert torch.equal(lp3.cpu(), lp1.cpu()[perm]) and torch.equal(g3.cpu(), g1.cpu()[perm])
    # steps
    ids = torch.arange(E, dtype=torch.int32)
    eps = torch.full((E,), 1e-3)
    L = torch.full((E,), 1.0)
    s0 = bf.init(th, seed=5, particle_ids=ids)
    s1, info, kept = bf.step(s0, eps, L, n_steps=4, seed=5, n_thinning=2, particle_ids=ids)
    s1b, info_b, _ = bf.step(s0, eps, L, n_steps=4, seed=5, n_thinning=2, particle_ids=ids)
    assert torch.equal(s1.position, s1b.position) and torch.equal(info.energy_change, info_b.energy_change)
    assert (s1.momentum.double().norm(dim=1) - 1).abs().max().item() < 1e-5
    assert kept.shape == (2, E, ospec.n_params) and torch.isfinite(kept).all() and torch.isfinite(info.energy_change).all()


def test_full_size_properties_b4(oracle):
    """BASELINE's B4 size (covertype-shaped: N=232404, F=54, [256 x 4, 7] softmax, 128 particles per GPU) on the
    layer-wise MFMA path (k_mm3), which walks the rows in chunks here: additivity over data, permutation equivariance
    over particles, generic-kernel agreement on a slice of rows and particles."""
    ospec, N, E = oracle.config_spec('B4')
    prob = oracle.synthetic_problem(ospec, N, E, seed=0)
    th = torch.from_numpy(prob['theta0'])
    ge = _engine(ospec, prob['X'], prob['y'])
    assert ge.grad_kernel == 'mfma_wide_bf16x3'
    lp1, g1 = ge.logpost_grad(th)
    assert torch.isfinite(lp1).all() and torch.isfinite(g1).all()
    h = 100000
    a = _engine(ospec, prob['X'][:h], prob['y'][:h]).logpost_grad(th)
    b = _engine(ospec, prob['X'][h:], prob['y'][h:]).logpost_grad(th)
    assert _rel((a[1] + b[1] + th.cuda()).cpu(), g1.cpu()) < 5e-5          # prior gradient -theta counted once
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(2))
    lp3, g3 = ge.logpost_grad(th[perm])
    assert _rel(lp3.cpu(), lp1.cpu()[perm]) < 1e-6 and _rel(g3.cpu(), g1.cpu()[perm]) < 1e-6
    # the single-launch generic kernel on 3 particles and the first 3000 rows.  Rows with a pre-activation within fp32 rounding
    # of the ReLU kink are left out for all three kernels (as in test_logpost_grad_matches_oracle): the kernels sum in different
    # orders, and a unit that is +1e-8 in one and -1e-8 in another flips ReLU' for its row (4e-3 absolute on a bias gradient)
    Xs, ys = prob['X'][:3000], prob['y'][:3000]
    _, zs, _ = oracle.mlp_forward(ospec, prob['theta0'][:3].astype(np.float64), Xs, keep=True)
    near = np.zeros(len(Xs), dtype=bool)
    for z in zs[:-1]:
        near |= (np.abs(z) < 3e-7 * np.abs(z).max()).any(axis=(0, 2))
    assert near.sum() < 30, near.sum()
    Xs, ys = np.ascontiguousarray(Xs[~near]), np.ascontiguousarray(ys[~near])
    r2 = _engine(ospec, Xs, ys, 'generic').logpost_grad(th[:3])
    for k in ('mfma_wide_bf16x3', 'gemm_f32'):          # the MFMA GEMMs, and the rocBLAS cross-check
        r1 = _engine(ospec, Xs, ys, k).logpost_grad(th[:3])
        assert _rel(r1[0].cpu(), r2[0].cpu()) < 2e-6 and _rel(r1[1].cpu(), r2[1].cpu()) < 2e-5, k
