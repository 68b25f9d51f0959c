"""A short Engine.step / Engine.tune run, bit for bit against the commit before the small-accumulator phase of k_grad_w64's
reduction was shortened (-m gpu).  That change keeps every expression and every order of addition, and the update launches
behind the gradient are untouched, so every bit of the state must stay -- through the first and last launches of a call, the
mid-step and record-point kinds and the tuner, which all read the slabs.

Shapes, at E = 3 particles (particle 2 repeats particle 0: same parameters, step size, L and particle id, and must equal it
bit for bit): nets [5, 64, 64, 2] and [5, 64, 64, 64, 2] on mfma_w64_bf16x3 (d = 4674 and 8834: two and three quads per thread
in the update launches, d % 4 = 2 so the tail elements run), N = 27 and 283 rows (S = 1 and S = 2 slabs per particle, a tail
block alone and a main-loop round).

Runs: 4 steps in one call with n_thinning = 2, and the same 4 steps as calls of 1 + 3 -- the first and last general-form
launches of a call, the mid-step and record-point kinds between them and the prefilled noise all run (tests/update_schedule.py
restates which launch is which).  One case runs Engine.tune for 3 steps (the warm-up kind).

tests/golden/step_edges_parent.json holds the SHA-256 of the float32 bytes of position, momentum, log-density, gradient and
kept samples (tune: the tuner's tensors as well) that a build of the parent commit returned on an MI355X for these inputs;
tests/golden/make_step_edges_digests.py wrote it and says how.  tests/test_gpu_w64_edges.py is the same check on the gradient
launch alone, over more forms.
"""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from tests import w64_schedule as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

DEV = 'cuda:0'
E = 3
KERNEL = 'mfma_w64_bf16x3'
NETS = [(5, (64, 64, 2)), (5, (64, 64, 64, 2))]
ROWS = {27: 1, 283: 2}                        # N -> slabs per particle at E = 3
CASES = [(net, N) for net in NETS for N in ROWS]
TUNE_CASE = (NETS[1], 283)
IDS = [0, 1, 0]
EPS = [2e-3, 3e-3, 2e-3]
LS = [20.0, 15.0, 20.0]
SEED = 11
N_STEPS, N_THINNING = 4, 2
GOLDEN = Path(__file__).resolve().parent / 'golden' / 'step_edges_parent.json'


def case_id(case):
    (F, hs), N = case
    return f'F{F}-h{len(hs) - 1}-N{N}'


def digest(arrays):
    """SHA-256 over the float32 bytes of the arrays, in order."""
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    return h.hexdigest()


def _engine(case):
    from mile_amd import ModelSpec
    from mile_amd.engine import Engine
    (F, hs), N = case
    form = (F, hs, KERNEL)
    _, X, y, theta = W.problem(form, N, E, W.seed_of(form, N))
    eng = Engine(ModelSpec(in_features=F, hidden_structure=hs), torch.from_numpy(X), torch.from_numpy(y), device=DEV, grad_kernel=KERNEL)
    assert eng.grad_kernel == KERNEL
    info = eng.grad_launch_info(E)
    assert info['kernel'] == 'k_grad_w64' and info['grid'] == (ROWS[N], E), (case_id(case), info)
    st = eng.init(torch.from_numpy(theta), seed=SEED, particle_ids=IDS)
    return eng, st


def _arrays(st, samples):
    """Everything particle-first: the kept samples as [E, n_kept, d]."""
    return [t.cpu().numpy() for t in (st.position, st.momentum, st.logdensity, st.logdensity_grad, samples.transpose(0, 1))]


def run_steps(case, calls):
    """N_STEPS steps from the initial state as consecutive calls of `calls` steps each: the arrays the digest is taken over."""
    eng, st = _engine(case)
    eps, L = torch.tensor(EPS), torch.tensor(LS)
    kept, done = [], 0
    for n in calls:
        st, _, smp = eng.step(st, eps, L, n, seed=SEED, step_offset=done, n_thinning=N_THINNING, particle_ids=IDS, want_info=False)
        if smp is not None:
            kept.append(smp)
        done += n
    torch.cuda.synchronize()
    assert done == N_STEPS
    samples = torch.cat(kept)
    assert samples.shape[0] == N_STEPS // N_THINNING
    return _arrays(st, samples)


def run_tune(case):
    """3 warm-up steps with the device tuner, the second and third past the masked phase: state and tuner tensors."""
    eng, st = _engine(case)
    d = st.position.shape[1]
    f32 = dict(dtype=torch.float32, device=DEV)
    tuner = {'step_size': torch.tensor(EPS, **f32), 'step_size_max': torch.full((E,), float('inf'), **f32),
             'time': torch.zeros(E, **f32), 'x_average': torch.zeros(E, **f32),
             'stream_weight': torch.zeros(E, **f32), 'stream_average': torch.zeros((E, 2, d), **f32)}
    eng.tune(st, tuner, torch.tensor(LS), 3, schedule_step0=0, n_mask_steps=1, schedule_total=4, desired_energy_var_start=0.5,
             desired_energy_var_end=0.1, trust_in_estimate=1.5, decay_rate=99 / 101, seed=SEED, step_offset=0, particle_ids=IDS)
    torch.cuda.synchronize()
    names = ('step_size', 'step_size_max', 'time', 'x_average', 'stream_weight', 'stream_average')
    return [t.cpu().numpy() for t in (st.position, st.momentum, st.logdensity, st.logdensity_grad)] + [tuner[k].cpu().numpy() for k in names]


RUNS = {'4': (4,), '1+3': (1, 3)}


def _check(key, arrays):
    assert all(np.isfinite(a).all() for a in arrays[:4]), key
    for a in arrays:      # the replica (every array is particle-first)
        assert a.shape[0] == E, (key, a.shape)
        assert np.array_equal(a[2], a[0]), (key, 'particle 2 differs from particle 0')
    want = json.loads(GOLDEN.read_text())
    got = digest(arrays)
    print(f'\nSTEPEDGE {key}: digest {got[:16]}  parent {want[key][:16]}')
    assert got == want[key], (key, 'the state differs from the parent build bit-wise')


@pytest.mark.parametrize('calls', list(RUNS), ids=[f'calls{c}' for c in RUNS])
@pytest.mark.parametrize('case', CASES, ids=[case_id(c) for c in CASES])
def test_step_edges(case, calls):
    _check(f'{case_id(case)}-steps{calls}', run_steps(case, RUNS[calls]))


def test_tune_edges():
    _check(f'{case_id(TUNE_CASE)}-tune3', run_tune(TUNE_CASE))
