"""mile_canonicalize_fcn on the GPU (-m gpu).

Every output float is an input float moved, possibly negated, so out, perm and sign are compared with array_equal against the
NumPy restatement tests/canon_ref.py (equal_nan where NaNs are placed): no tolerance anywhere.  The shapes (canon_ref.CASES)
are the smallest at which each part can go wrong: a full wave per layer, twelve layers (lexicographic layout), width 1, no
hidden layer, widths above a wave in a draw near the LDS limit, a draw that takes the row-tiled form."""
import json
import subprocess
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import canon_ref as CR
from tests import fdiag_ref as F

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ROOT = Path(__file__).resolve().parents[1]
DEV = 'cuda:0'
FIVE = ('wcv', 'bcv', 'ess', 'crhat', 'rhat')
CASE_COMBOS = [(n, k, s) for n in CR.CASES for k, s in CR.case_combos(n)]


def _t(a):
    return torch.from_numpy(np.array(a))                  # a copy: the shared cases are read-only


def _device(spec, theta, key, sign, index=True):
    from mile_amd import metrics as M
    res = M.canonicalize(spec, _t(theta).to(DEV), key, sign, return_perm=index)
    assert M.LAST_CANON_PATH == 'library'
    return tuple(t.cpu().numpy() for t in res) if index else res.cpu().numpy()


def _same(got, ref, what, equal_nan=False):
    for g, r, name, dt in zip(got, ref, ('out', 'perm', 'sign'), (np.float32, np.int32, np.int8)):
        assert g.dtype == dt and g.shape == r.shape, (what, name, g.dtype, g.shape, r.shape)
        assert np.array_equal(g, r, equal_nan=equal_nan and name == 'out'), (what, name, int((g != r).sum()))


@pytest.mark.parametrize('name,key,sign', CASE_COMBOS)
def test_cases_equal_the_restatement(name, key, sign):
    spec, theta = CR.case_spec(name), CR.case_draws(name)
    got = _device(spec, theta, key, sign)
    _same(got, CR.case_canonical(name, key, sign), (name, key, sign))
    if name == 'nohidden':                                # H = 0: a copy, and null perm / sign
        assert got[1].shape == (theta.shape[0], 0) and np.array_equal(_device(spec, theta, key, sign, index=False), theta)


@pytest.mark.parametrize('key,sign', CR.COMBOS)
def test_permutation_case_diagnostics(key, sign):
    """[3, 64, d] draws around one mode, chains 1 and 2 permuted: canonical_diagnostics equals chain_diagnostics of the
    restatement's canonical draws bit for bit; its max rhat is below 1.1 where the raw draws' is above 2 (fp64: 1.0370, 2.4091)."""
    from mile_amd import metrics as M
    spec, theta = CR.permutation_spec(), CR.permutation_draws()
    ref_out, ref_perm, _ = CR.permutation_canonical(key, sign)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        got = M.canonical_diagnostics(spec, _t(theta).to(DEV), 2, key=key, sign=sign)
        assert M.LAST_CANON_PATH == 'library' and M.LAST_DIAG_PATH == 'library'
        want = M.chain_diagnostics(_t(ref_out).to(DEV), 2)
        raw = M.chain_diagnostics(_t(theta).to(DEV), 2)
    for k in FIVE:
        assert np.array_equal(got[k].cpu().numpy(), want[k].cpu().numpy(), equal_nan=True), k
    assert got['switches'].dtype == torch.int64 and np.array_equal(got['switches'].cpu().numpy(), CR.switches(ref_perm, F.PERM_WIDTHS[:-1]))
    c_max, r_max = float(got['rhat'].max()), float(raw['rhat'].max())
    print(f'CANON permutation {key} sign={sign}: parameter rhat max raw {r_max:.4f} canonical {c_max:.4f}  '
          f'above 1.1: {int((got["rhat"] > 1.1).sum())} of {got["rhat"].numel()}')
    assert r_max > 2.0 and c_max < 1.1


def test_specials_on_the_device():
    """Two identical units, -0.0 / +0.0 biases, +-inf, and one draw with NaN biases: NaN last, the other draws bit for bit."""
    spec, theta = CR.specials()
    clean = np.delete(theta, 2, axis=0)
    for key, sign in CR.COMBOS:
        got = _device(spec, theta, key, sign)
        _same(got, CR.canonicalize(spec, theta, key, sign), (key, sign), equal_nan=True)
        _same(tuple(np.delete(g, 2, axis=0) for g in got), CR.canonicalize(spec, clean, key, sign), (key, sign, 'clean'))


@pytest.mark.parametrize('name,key,sign', [('perm', 'bias', True), ('w64x3', 'norm', False), ('wide', 'bias', False)])
def test_the_function_is_unchanged_on_the_device(name, key, sign):
    """Engine.predict of the canonical draws and of the raw draws: both within the bound of tests/test_gpu_predict.py,
    max|out - ref| < 1e-4 * max(1, max|ref|), of the fp64 forward of the RAW draws."""
    from mile_amd.engine import Engine
    spec, theta = CR.case_spec(name), CR.case_draws(name)
    ospec = O.ModelSpec(spec.in_features, spec.hidden_structure, activation=spec.activation, task=spec.task)
    prob = O.synthetic_problem(ospec, 16, 1, seed=2)
    eng = Engine(spec, _t(prob['X']), _t(prob['y']), device=DEV)
    ref = O.mlp_forward(ospec, theta.astype(np.float64), prob['X'].astype(np.float64))
    canon = eng.canonicalize(_t(theta), key, sign)
    assert canon.is_cuda and np.array_equal(canon.cpu().numpy(), CR.case_canonical(name, key, sign)[0])
    scale = max(1.0, np.abs(ref).max())
    for tag, th in (('raw', _t(theta)), ('canonical', canon)):
        err = np.abs(eng.predict(th, _t(prob['X'])).cpu().numpy().astype(np.float64) - ref).max()
        print(f'CANON predict {name} {tag}: max|out - ref| = {err:.3e}, bound {1e-4 * scale:.3e}')
        assert err < 1e-4 * scale, (tag, err)


@pytest.mark.parametrize('name', ['w64x3', 'tiled'])
def test_index_outputs_and_batch_size_change_no_bit(name):
    """perm / sign null or given: the same out.  The same draws as M and as the first rows of a batch of 40: the same rows."""
    spec = CR.case_spec(name)
    M_ = CR.CASES[name][4]
    many = CR.random_draws(spec, 40, seed=21)
    many[:M_] = CR.case_draws(name)
    for key in CR.KEYS:
        ref = CR.case_canonical(name, key, False)
        assert np.array_equal(_device(spec, many[:M_], key, False, index=False), ref[0])
        got = _device(spec, many, key, False)
        _same(tuple(g[:M_] for g in got), ref, (name, key))
        _same(got, CR.canonicalize(spec, many, key, False), (name, key, 40))


def test_misaligned_draws():
    """d = 122 is no multiple of 4 and the batch starts 1, 2 and 3 floats past a 16-byte boundary: head, body and tail of the
    16-byte staging loads."""
    from mile_amd import metrics as M
    spec = CR.permutation_spec()
    theta = CR.random_draws(spec, 9, seed=31)
    ref = CR.canonicalize(spec, theta, 'norm', True)
    for shift in (1, 2, 3):
        buf = torch.zeros(9 * spec.n_params + 8, device=DEV)
        view = buf[shift:shift + 9 * spec.n_params].view(9, spec.n_params)
        view.copy_(_t(theta))
        assert view.data_ptr() % 16 == 4 * shift
        got = M._library_canonicalize(spec, view, 'norm', True, True)
        _same(tuple(t.cpu().numpy() for t in got), ref, shift)
        assert bool((buf[:shift] == 0).all()) and bool((buf[shift + 9 * spec.n_params:] == 0).all())


def test_evaluate_cli_canonical_diagnostics(tmp_path):
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
    assert not any(k.startswith('cdiag_') for k in before)
    r = subprocess.run([sys.executable, str(ROOT / 'evaluate.py'), '-e', str(exp), '--diagnostics', '--canonical-diagnostics',
                        '--canonical-key', 'norm'], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = json.loads((exp / 'metrics.json').read_text())
    assert {k: v for k, v in m.items() if not k.startswith('cdiag_')} == before            # the other keys are unchanged
    diag = [k for k in m if k.startswith('diag_')]
    assert diag and all('c' + k in m for k in diag)                                        # cdiag_* mirrors diag_* one for one
    C_, S, d = m['n_chains'], m['n_samples'], None
    z = np.load(exp / 'canonical_diagnostics.npz')
    assert sorted(z.files) == ['bcv', 'crhat', 'ess', 'rhat', 'switches', 'wcv']
    d = z['rhat'].shape[0]
    n_hidden = z['switches'].shape[1]
    assert z['ess'].shape == z['crhat'].shape == (C_, d) and z['wcv'].shape == z['bcv'].shape == (d,) and z['switches'].shape == (C_, n_hidden)
    assert n_hidden >= 1 and z['switches'].dtype == np.int64 and (z['switches'] >= 0).all() and (z['switches'] <= S - 1).all()
    assert m['cdiag_key'] == 'norm' and m['cdiag_sign'] is False and m['cdiag_n_splits'] == 2
    assert m['cdiag_rhat_max'] == float(np.nanmax(z['rhat'])) and m['cdiag_ess_min'] == float(np.nanmin(z['ess']))
    for l in range(n_hidden):
        assert m[f'cdiag_switch_rate_layer{l}'] == pytest.approx(float(np.mean(z['switches'][:, l] / (S - 1))), rel=1e-12)
    assert set(m['cdiag_ess_layer_mean']) == set(m['diag_ess_layer_mean'])
