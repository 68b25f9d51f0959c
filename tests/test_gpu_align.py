"""mile_align_fcn on the GPU (-m gpu).

The similarities are sums of exact products added in a fixed order and the solver only adds, subtracts and compares, so out, perm,
sign, dropped and the fp64 scores are compared with array_equal against the NumPy restatement tests/align_ref.py: no tolerance
anywhere.  The shapes (align_ref.CASES) are the smallest at which each part can go wrong: a full wave per layer with three chained
layers, two columns per lane, widths below and across a wave that are no powers of two, assignments that do not recover the
original, twelve layers (lexicographic layout), width 1, no hidden layer."""
import json
import subprocess
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import align_ref as A
from tests import canon_ref as CR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ROOT = Path(__file__).resolve().parents[1]
DEV = 'cuda:0'
CASE_SIGNS = [(n, s) for n in A.CASES for s in A.case_signs(n)]
NAMES = ('out', 'perm', 'sign', 'score', 'dropped')
DTYPES = (np.float32, np.int32, np.int8, np.float64, np.int32)


def _t(a):
    return torch.from_numpy(np.array(a))                  # a copy: the shared cases are read-only


def _device(spec, theta, reference, sign, index=True, score=True):
    from mile_amd import metrics as M
    res = M._library_align(spec, _t(theta).to(DEV), _t(reference).to(DEV), sign, index, score)
    return tuple(t.cpu().numpy() if t is not None else None for t in res)


def _same(got, ref, what, equal_nan=False):
    for g, r, name, dt in zip(got, ref, NAMES, DTYPES):
        assert g.dtype == dt and g.shape == r.shape, (what, name, g.dtype, g.shape, r.shape)
        if name == 'score':                               # as fp64 bits; a dropped draw's scores are NaN in both
            nan = np.isnan(r)
            assert nan.any() <= equal_nan and np.array_equal(np.isnan(g), nan), (what, name)
            assert np.array_equal(np.ascontiguousarray(g[~nan]).view(np.int64), np.ascontiguousarray(r[~nan]).view(np.int64)), (what, name)
        else:
            assert np.array_equal(g, r, equal_nan=equal_nan and name == 'out'), (what, name, int((g != r).sum()))


@pytest.mark.parametrize('name,sign', CASE_SIGNS)
def test_cases_equal_the_restatement(name, sign):
    from mile_amd import metrics as M
    spec = A.case_spec(name)
    centre, orig, moved = A.case_data(name)
    got = _device(spec, moved, centre, sign)
    _same(got, A.case_aligned(name, sign), (name, sign))
    if name in A.RECOVERED and sign == (spec.activation == 'tanh'):           # the unpermuted draws come back bit for bit
        assert np.array_equal(got[0], orig) and not np.array_equal(moved, orig)
    if name == 'nohidden':                                                      # H = 0: a copy
        assert got[1].shape == (moved.shape[0], 0) and got[3].shape == (moved.shape[0], 0) and np.array_equal(got[0], moved)
    res = M.align(spec, _t(moved).to(DEV), _t(centre).to(DEV), sign=sign)       # the public path takes the library
    assert M.LAST_ALIGN_PATH == 'library' and np.array_equal(res['theta'].cpu().numpy(), got[0])
    assert np.array_equal(res['reference'].cpu().numpy(), centre)


def test_batch_size_and_optional_outputs_change_no_bit():
    """7 draws alone and as the first 7 of 40, with and without perm / sign / score: the same bits."""
    spec = A.case_spec('w16')
    centre, _, moved = A.case_data('w16')
    ref = A.case_aligned('w16', False)
    _same(_device(spec, moved, centre, False), ref, 40)
    alone = _device(spec, moved[:7], centre, False)
    _same(alone, tuple(r[:7] for r in ref), 7)
    bare = _device(spec, moved[:7], centre, False, index=False, score=False)
    assert bare[1] is None and bare[2] is None and bare[3] is None
    assert np.array_equal(bare[0], ref[0][:7]) and np.array_equal(bare[4], ref[4][:7])
    half = _device(spec, moved, centre, False, index=True, score=False)
    assert half[3] is None and np.array_equal(half[0], ref[0]) and np.array_equal(half[1], ref[1])


def test_misaligned_draws():
    """theta and the reference start 1 float past a 16-byte boundary (d = 122 is no multiple of 4): the same bits."""
    from mile_amd import metrics as M
    spec = A.case_spec('sep')
    centre, _, moved = A.case_data('sep')
    ref = A.case_aligned('sep', True)
    n = moved.size
    buf = torch.zeros(n + 8, device=DEV)
    view = buf[1:1 + n].view(moved.shape)
    view.copy_(_t(moved))
    rbuf = torch.zeros(centre.size + 8, device=DEV)
    rview = rbuf[1:1 + centre.size]
    rview.copy_(_t(centre))
    assert view.data_ptr() % 16 == 4 and rview.data_ptr() % 16 == 4
    got = M._library_align(spec, view, rview, True)
    _same(tuple(t.cpu().numpy() for t in got), ref, 'shift 1')
    assert bool((buf[:1] == 0).all()) and bool((buf[1 + n:] == 0).all())


def test_a_nan_draw_is_dropped_and_copied_on_the_device():
    spec = A.case_spec('sep')
    centre, _, moved = A.case_data('sep')
    theta = np.array(moved[:5])
    off = {n.split('.', 1)[1]: o for n, o, _ in spec.leaves()}
    theta[1, off['layer1.kernel'] + 3] = np.nan                                 # layer 0 solves, layer 1 does not
    theta[3, off['layer0.bias'] + 2] = np.inf
    for sign in (False, True):
        ref = A.align(spec, theta, centre, sign)
        assert ref[4].tolist() == [0, 1, 0, 1, 0]
        _same(_device(spec, theta, centre, sign), ref, sign, equal_nan=True)


@pytest.mark.parametrize('name', ['sep', 'w64x3', 'w128'])
def test_the_function_is_unchanged_on_the_device(name):
    """Engine.predict of the aligned draws and of the raw draws: both within the bound of tests/test_gpu_canon.py,
    max|out - ref| < 1e-4 * max(1, max|ref|), of the fp64 forward of the RAW draws."""
    from mile_amd.engine import Engine
    spec = A.case_spec(name)
    centre, _, moved = A.case_data(name)
    sign = spec.activation == 'tanh'
    ospec = O.ModelSpec(spec.in_features, spec.hidden_structure, activation=spec.activation, task=spec.task)
    prob = O.synthetic_problem(ospec, 16, 1, seed=2)
    eng = Engine(spec, _t(prob['X']), _t(prob['y']), device=DEV)
    ref = O.mlp_forward(ospec, moved.astype(np.float64), prob['X'].astype(np.float64))
    aligned, perm, sgn, score, dropped = eng.align(_t(moved), _t(centre), sign, return_index=True, return_score=True)
    want = A.case_aligned(name, sign)
    assert aligned.is_cuda and np.array_equal(aligned.cpu().numpy(), want[0]) and np.array_equal(perm.cpu().numpy(), want[1])
    assert np.array_equal(score.cpu().numpy(), want[3]) and not bool(dropped.any())
    assert np.array_equal(eng.align(_t(moved), _t(centre), sign).cpu().numpy(), want[0])
    scale = max(1.0, np.abs(ref).max())
    for tag, th in (('raw', _t(moved)), ('aligned', aligned)):
        err = np.abs(eng.predict(th, _t(prob['X'])).cpu().numpy().astype(np.float64) - ref).max()
        print(f'ALIGN predict {name} {tag}: max|out - ref| = {err:.3e}, bound {1e-4 * scale:.3e}')
        assert err < 1e-4 * scale, (tag, err)


@pytest.mark.parametrize('sign', [False, True])
def test_permutation_case_diagnostics(sign):
    """[3, 64, d] draws around one mode, chains 1 and 2 permuted, through metrics.aligned_diagnostics on the device path: max rhat
    below 1.1 where the raw draws' is above 2, and no chain ever changes its matching."""
    from mile_amd import metrics as M
    spec, theta = CR.permutation_spec(), CR.permutation_draws()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        got = M.aligned_diagnostics(spec, _t(theta).to(DEV), 2, reference='first', rounds=2, sign=sign)
        assert M.LAST_ALIGN_PATH == 'library' and M.LAST_DIAG_PATH == 'library'
        raw = M.chain_diagnostics(_t(theta).to(DEV), 2)
    a_max, r_max = float(got['rhat'].max()), float(raw['rhat'].max())
    print(f'ALIGN permutation sign={sign}: parameter rhat max raw {r_max:.4f} aligned {a_max:.4f}  '
          f'above 1.1: {int((got["rhat"] > 1.1).sum())} of {got["rhat"].numel()}  switches {got["switches"].tolist()}')
    assert r_max > 2.0 and a_max < 1.1
    assert got['switches'].dtype == torch.int64 and got['switches'].shape == (3, 2) and bool((got['switches'] == 0).all())
    assert got['dropped'] == 0 and bool(torch.isfinite(got['score_mean']).all())
    # round 1 on the device is the restatement's round 1, bit for bit
    one = M.align(spec, _t(theta).to(DEV), 'first', rounds=1, sign=sign)
    want = A.permutation_aligned(sign, rounds=1)
    assert np.array_equal(one['theta'].cpu().numpy(), want[0]) and np.array_equal(one['perm'].cpu().numpy(), want[1])
    assert np.array_equal(one['score'].cpu().numpy(), want[3])


def test_evaluate_cli_aligned_diagnostics(tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=80, n_chains=4)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, str(ROOT / 'train.py'), '-c', str(tmp_path / 'cfg.yaml'), '-d', '1'],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    exp = tmp_path / 'smoke_synthetic'
    r = subprocess.run([sys.executable, str(ROOT / 'evaluate.py'), '-e', str(exp), '--diagnostics'], capture_output=True, text=True,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    before = json.loads((exp / 'metrics.json').read_text())
    assert not any(k.startswith('adiag_') for k in before)
    r = subprocess.run([sys.executable, str(ROOT / 'evaluate.py'), '-e', str(exp), '--diagnostics', '--aligned-diagnostics',
                        '--tail-diagnostics'], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = json.loads((exp / 'metrics.json').read_text())
    assert {k: v for k, v in m.items() if not k.startswith(('adiag_', 'dtail_'))} == before     # the other keys are unchanged
    diag = [k for k in m if k.startswith('diag_')]
    assert diag and all('a' + k in m for k in diag)                                        # adiag_* mirrors diag_* one for one
    tails = [k for k in m if k.startswith('dtail_')]
    assert tails and all('adiag_tail_' + k[len('dtail_'):] in m for k in tails)
    C_, S = m['n_chains'], m['n_samples']
    z = np.load(exp / 'aligned_diagnostics.npz')
    assert sorted(z.files) == ['bcv', 'crhat', 'ess', 'reference', 'rhat', 'score_mean', 'scores', 'switches', 'wcv']
    d = z['rhat'].shape[0]
    n_hidden = z['switches'].shape[1]
    assert z['ess'].shape == z['crhat'].shape == (C_, d) and z['wcv'].shape == z['bcv'].shape == z['reference'].shape == (d,)
    assert z['switches'].shape == (C_, n_hidden) and z['scores'].shape == (C_, S, n_hidden) and z['score_mean'].shape == (n_hidden,)
    assert n_hidden >= 1 and z['switches'].dtype == np.int64 and (z['switches'] >= 0).all() and (z['switches'] <= S - 1).all()
    assert z['reference'].dtype == np.float32 and z['scores'].dtype == np.float64 and np.isfinite(z['scores']).all()
    assert m['adiag_dropped'] == 0 and m['adiag_reference'] == 'first' and m['adiag_rounds'] == 2 and m['adiag_sign'] is False
    assert m['adiag_n_splits'] == 2
    assert m['adiag_rhat_max'] == float(np.nanmax(z['rhat'])) and m['adiag_ess_min'] == float(np.nanmin(z['ess']))
    for l in range(n_hidden):
        assert m[f'adiag_switch_rate_layer{l}'] == pytest.approx(float(np.mean(z['switches'][:, l] / (S - 1))), rel=1e-12)
        assert m[f'adiag_score_mean_layer{l}'] == pytest.approx(float(z['score_mean'][l]), rel=1e-12)
    assert set(m['adiag_ess_layer_mean']) == set(m['diag_ess_layer_mean'])
