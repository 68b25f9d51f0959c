"""The record launch's O-step noise drawn one launch early (-m gpu).

In a sampling call every mid-step update launch (k_update_fast, UPD_KIND_MID) runs E extra workgroups that write the
Philox normals of the record launch that follows it; the record launch reads them through its explicit-noise path.
MILE_DEBUG bit 128 turns that off.  Both paths draw the same counters, so every output must be bit-identical; the
library's prefill counter (mile_debug_prefill_count) shows that the prefill actually ran."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

NO_PREFILL = '128'


def _engine(oracle, F, hs, X, y, kernel='auto'):
    from mile_amd import ModelSpec
    from mile_amd.engine import Engine
    ospec = oracle.ModelSpec(F, hs)
    return Engine(ModelSpec(in_features=ospec.in_features, hidden_structure=ospec.hidden_structure),
                  torch.from_numpy(np.asarray(X)), torch.from_numpy(np.asarray(y)), device='cuda:0', grad_kernel=kernel)


def _run(eng, prob, sl, ids, refresh, chunks, seed=11, offset=4, n_thinning=3):
    """Consecutive step calls (chunk boundaries between them); everything they return, on the host."""
    th, eps, L = (torch.from_numpy(prob[k])[sl] for k in ('theta0', 'eps', 'L'))
    s = eng.init(th, seed=seed, particle_ids=ids[sl])
    out = []
    for c in chunks:
        s, info, kept = eng.step(s, eps, L, n_steps=c, seed=seed, step_offset=offset, n_thinning=n_thinning,
                                 particle_ids=ids[sl], refresh=refresh)
        offset += c
        out += [s.position, s.momentum, s.logdensity, s.logdensity_grad,
                info.logdensity, info.kinetic_change, info.energy_change]
        if kept is not None:   # (a call that crosses no thinning point keeps nothing)
            out.append(kept)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


@pytest.mark.parametrize('F,hs,kernel', [
    (5, (64, 64, 64, 2), 'auto'),           # B2's net (mfma_w64_bf16x3), d % 4 == 2
    (5, (64, 64, 2), 'mfma_w64_bf16x3'),
    (4, (8, 6, 2), 'generic'),              # d = 108, d % 4 == 0
    (4, (7, 6, 2), 'generic'),              # d = 97: one tail element, scalar (AL = 1) stores
    (6, (7, 6, 2), 'generic'),              # d = 111: three tail elements
])
@pytest.mark.parametrize('refresh', ['O-step-O', 'step-O'])
def test_prefilled_noise_is_bit_identical(oracle, monkeypatch, F, hs, kernel, refresh):
    ospec = oracle.ModelSpec(F, hs)
    prob = oracle.synthetic_problem(ospec, 150, 9, seed=3)
    eng = _engine(oracle, F, hs, prob['X'], prob['y'], kernel)
    ids = torch.arange(40, 49, dtype=torch.int32)
    for sl in (slice(0, 9), slice(2, 5)):   # the full ensemble, then fewer particles than the workspace holds
        for chunks in ((1,), (6, 1, 5)):     # a one-step call (its only record launch is the call's last), several calls
            monkeypatch.delenv('MILE_DEBUG', raising=False)
            n0 = eng.debug_prefill_count()
            on = _run(eng, prob, sl, ids, refresh, chunks)
            # every step's mid-step launch prefilled the noise of the record launch after it
            assert eng.debug_prefill_count() - n0 == sum(chunks)
            monkeypatch.setenv('MILE_DEBUG', NO_PREFILL)
            n0 = eng.debug_prefill_count()
            off = _run(eng, prob, sl, ids, refresh, chunks)
            assert eng.debug_prefill_count() == n0
            monkeypatch.delenv('MILE_DEBUG')
            assert len(on) == len(off)
            for k, (a, b) in enumerate(zip(on, off)):
                assert torch.equal(a, b), (sl, chunks, k)
    # the last comparison (three calls) included kept samples, and the trajectory moved
    assert len(on) == 3 * 7 + 2 and not torch.equal(on[0], torch.from_numpy(prob['theta0'])[2:5])


def test_prefilled_noise_matches_explicit_philox_noise(oracle, monkeypatch):
    """The prefilled numbers are the counter RNG's: a run fed mile_debug_noise's draws as explicit noise is the same run."""
    F, hs = 5, (64, 64, 64, 2)
    ospec = oracle.ModelSpec(F, hs)
    prob = oracle.synthetic_problem(ospec, 120, 4, seed=5)
    eng = _engine(oracle, F, hs, prob['X'], prob['y'])
    ids = torch.arange(7, 11, dtype=torch.int32)
    th, eps, L = (torch.from_numpy(prob[k]) for k in ('theta0', 'eps', 'L'))
    seed, off, T = 21, 2, 5
    monkeypatch.delenv('MILE_DEBUG', raising=False)
    s0 = eng.init(th, seed=seed, particle_ids=ids)
    n0 = eng.debug_prefill_count()
    a, info_a, _ = eng.step(s0, eps, L, n_steps=T, seed=seed, step_offset=off, particle_ids=ids)
    assert eng.debug_prefill_count() - n0 == T
    # the step's slot layout: noise[i, 0] = stage 0 of global step off + i, noise[i, 1] = stage 1
    z = torch.stack([torch.stack([eng.debug_noise(seed, 4, off + i, k, particle_ids=ids).cpu() for k in (0, 1)])
                     for i in range(T)])
    n0 = eng.debug_prefill_count()
    b, info_b, _ = eng.step(s0, eps, L, n_steps=T, noise=z, particle_ids=ids)
    torch.cuda.synchronize()
    assert eng.debug_prefill_count() == n0             # explicit noise: nothing to prefill
    assert torch.equal(a.position.cpu(), b.position.cpu()) and torch.equal(a.momentum.cpu(), b.momentum.cpu())
    assert torch.equal(info_a.energy_change.cpu(), info_b.energy_change.cpu())
