"""mile_predict / Engine.predict: the raw outputs of every evaluation kernel against the fp64 forwards, their consistency
with pointwise_loglik, S beyond the gridDim.y limit, NaN pass-through and the new evaluate.py keys (-m gpu).

The bound on the raw outputs is the project's bound on pointwise_loglik for the same kernels:
max|out - ref| < 1e-4 * max(1, max|ref|) (2e-3 for lenet_bf16)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import lenet_oracle as LN
from oracle import mclmc_oracle as O
from tests import attn_pre_ref as RP
from tests import attn_ref as RA
from tests import lenetti_ref as RL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ROOT = Path(__file__).resolve().parents[1]
DEV = 'cuda:0'


def _assert_close(tag, got, ref, bound=1e-4):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    err, scale = np.abs(got - ref).max(), max(1.0, np.abs(ref).max())
    print(f'{tag}: max|out - ref| = {err:.3e}, max|ref| = {np.abs(ref).max():.3e}, bound {bound * scale:.3e}')
    assert err < bound * scale, (tag, err, scale)


def _fcn_engine(ospec, prob, kernel):
    from mile_amd import ModelSpec
    from mile_amd.engine import Engine
    spec = ModelSpec(ospec.in_features, ospec.hidden_structure, activation=ospec.activation, task=ospec.task)
    eng = Engine(spec, torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV, grad_kernel=kernel)
    assert eng.grad_kernel == kernel
    return eng


FCN_CASES = [
    # kernel, F, hidden_structure, activation, task
    ('generic', 5, (24, 12, 2), 'tanh', 'regr'),
    ('generic', 7, (24, 12, 5), 'relu', 'classification'),
    ('mfma_w64', 5, (64, 64, 2), 'relu', 'regr'),
    ('mfma_w64', 11, (64, 2), 'relu', 'regr'),                      # 9..16 features: the two-quad input form
    ('mfma_w64_bf16x3', 5, (64, 64, 64, 2), 'relu', 'regr'),
    ('mfma_narrow_f32', 5, (16, 16, 2), 'relu', 'regr'),
    ('mfma_narrow_f32', 8, (32, 32, 7), 'sigmoid', 'classification'),
    ('mfma_wide_bf16x3', 9, (128, 96, 2), 'relu', 'regr'),
    ('mfma_wide_bf16x3', 9, (128, 96, 6), 'tanh', 'classification'),
    ('gemm_f32', 9, (128, 96, 2), 'relu', 'regr'),
    ('gemm_f32', 9, (128, 96, 6), 'tanh', 'classification'),
    ('mfma_w128_bf16', 5, (128, 128, 2), 'relu', 'regr'),           # its evaluation is the fp32-faithful wide path
]


@pytest.mark.parametrize('kernel,F,hs,act,task', FCN_CASES, ids=[f'{c[0]}-{c[4]}-{c[1]}' for c in FCN_CASES])
def test_fcn_outputs_match_fp64(kernel, F, hs, act, task):
    ospec = O.ModelSpec(F, hs, activation=act, task=task)
    prob = O.synthetic_problem(ospec, 64, 5, seed=3, theta_scale=0.3)
    test = O.synthetic_problem(ospec, 301, 1, seed=4)
    eng = _fcn_engine(ospec, prob, kernel)
    out = eng.predict(torch.from_numpy(prob['theta0']), torch.from_numpy(test['X']))
    ref = O.mlp_forward(ospec, prob['theta0'].astype(np.float64), test['X'].astype(np.float64))
    assert out.shape == (5, 301, hs[-1])
    _assert_close(kernel, out, ref)


@pytest.mark.parametrize('K,act,task', [(2, 'relu', 'regr'), (3, 'tanh', 'classification')])
@pytest.mark.parametrize('kernel,S,Sc', [('mfma_wide_bf16x3', 515, 512), ('gemm_f32', 1027, 1024)])
def test_fcn_evaluation_walks_row_and_sample_chunks(monkeypatch, kernel, S, Sc, K, act, task):
    """launch_fwd_wide and launch_fwd_gemm beyond one row chunk and one sample chunk: 37 rows in chunks of 16, 16 and 5, S samples
    in one chunk of Sc (512 / 1024) and a second of 3.  [9 -> 24 -> 17 -> K] pads to 24, 24, 8 columns, so the two ping-pong
    buffers change their leading dimension between layers.  The first and last sample of each sample chunk on their own."""
    monkeypatch.setenv('MILE_GEMM_ROWS', '16')                   # read by the library in every evaluation call
    ospec = O.ModelSpec(9, (24, 17, K), activation=act, task=task)
    prob = O.synthetic_problem(ospec, 64, S, seed=3, theta_scale=0.3)
    test = O.synthetic_problem(ospec, 37, 1, seed=4)
    eng = _fcn_engine(ospec, prob, kernel)
    theta, X, y = torch.from_numpy(prob['theta0']), torch.from_numpy(test['X']), torch.from_numpy(test['y'])
    out = eng.predict(theta, X)
    pw = eng.pointwise_loglik(theta, X, y)
    ref = O.mlp_forward(ospec, prob['theta0'].astype(np.float64), test['X'].astype(np.float64))
    ref_ll = O.pointwise_loglik_raw(ospec, ref, test['y'].astype(np.float64))[0]
    assert out.shape == (S, 37, K) and pw.shape == (S, 37) and np.isfinite(ref_ll).all()
    _assert_close(f'{kernel} predict', out, ref)
    _assert_close(f'{kernel} loglik', pw, ref_ll)
    for smp in (0, Sc - 1, Sc, S - 1):
        _assert_close(f'{kernel} predict sample {smp}', out[smp], ref[smp])
        _assert_close(f'{kernel} loglik sample {smp}', pw[smp], ref_ll[smp])


@pytest.mark.parametrize('kernel,bound', [('lenet_f32', 1e-4), ('lenet_bf16', 2e-3)])
@pytest.mark.parametrize('C,H,W,K,act,task', [(1, 28, 28, 10, 'relu', 'classification'), (2, 13, 17, 2, 'tanh', 'regr')])
def test_lenet_outputs_match_fp64(kernel, bound, C, H, W, K, act, task):
    from mile_amd import LeNetSpec
    from mile_amd.engine import Engine
    ospec = LN.LeNetSpec(C, H, W, K, activation=act, task=task)
    prob = LN.synthetic_problem(ospec, 37, 3, seed=3)
    spec = LeNetSpec(C, H, W, K, activation=act, task=task)
    eng = Engine(spec, torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV, grad_kernel=kernel)
    assert eng.grad_kernel == kernel
    out = eng.predict(torch.from_numpy(prob['theta0']), torch.from_numpy(prob['X']))          # 4-D images are flattened
    ref = LN.forward(ospec, prob['theta0'].astype(np.float64), prob['X'])
    assert out.shape == (3, 37, K)
    _assert_close(kernel, out, ref, bound)


@pytest.mark.parametrize('C,H,W,K,task', [(1, 28, 28, 10, 'classification'), (3, 9, 11, 2, 'regr')])
def test_lenetti_outputs_match_fp64(C, H, W, K, task):
    from mile_amd import LeNettiSpec
    from mile_amd.engine import Engine
    ospec = RL.LeNettiSpec(C, H, W, K, activation='tanh', task=task)
    prob = RL.synthetic_problem(ospec, 20, 5, seed=6)
    test = RL.synthetic_problem(ospec, 301, 1, seed=7)
    eng = Engine(LeNettiSpec(C, H, W, K, activation='tanh', task=task), torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV)
    assert eng.grad_kernel == 'lenetti_f32'
    out = eng.predict(torch.from_numpy(prob['theta0']), torch.from_numpy(test['X']))
    ref = RL.forward(ospec, prob['theta0'].astype(np.float64), test['X'])
    assert out.shape == (5, 301, K)
    _assert_close('lenetti', out, ref)


def test_attention_outputs_match_fp64():
    from mile_amd.engine import Engine
    from mile_amd.spec import AttentionSpec
    spec = AttentionSpec(100, 30, 16, 4, 16, n_classes=3, projection_dim=(8,), use_bias=True, prior='Normal', prior_scale=0.2)
    prob = RA.synthetic_problem(spec, 20, 5, seed=6)
    test = RA.synthetic_problem(spec, 301, 1, seed=7)
    eng = Engine(spec, torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV)
    assert eng.grad_kernel == 'attn_f32'
    out = eng.predict(torch.from_numpy(prob['theta0']), torch.from_numpy(test['X']))
    ref = np.stack([RA._forward(spec, RA.unpack(spec, t), test['x'])['logits'] for t in prob['theta0']])
    assert out.shape == (5, 301, 3)
    _assert_close('attn', out, ref)


def test_wide_attention_outputs_match_fp64():
    from mile_amd.engine import Engine
    from mile_amd.spec import WideAttentionSpec
    spec = WideAttentionSpec(100, 30, 72, 4, 16, n_classes=3, projection_dim=(8,), use_bias=True, prior='Normal', prior_scale=0.2)
    prob = RA.synthetic_problem(spec, 20, 5, seed=6)
    test = RA.synthetic_problem(spec, 301, 1, seed=7)
    eng = Engine(spec, torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV)
    assert eng.grad_kernel == 'attn_wide_f32'
    out = eng.predict(torch.from_numpy(prob['theta0']), torch.from_numpy(test['X']))
    ref = np.stack([RA._forward(spec, RA.unpack(spec, t), test['x'])['logits'] for t in prob['theta0']])
    _assert_close('attn_wide', out, ref)


def test_pretrained_attention_outputs_match_fp64():
    from mile_amd.engine import Engine
    from mile_amd.spec import PretrainedAttentionSpec
    spec = PretrainedAttentionSpec(100, 30, 72, 4, 16, n_classes=3, projection_dim=(8,), use_bias=True, prior='Normal', prior_scale=0.2)
    prob = RP.synthetic_problem(spec, 20, 5, seed=6)
    test = RP.synthetic_problem(spec, 301, 1, seed=7)
    eng = Engine(spec, torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV, tables=(prob['emb'], prob['pos']))
    assert eng.grad_kernel == 'attn_pre_f32'
    out = eng.predict(torch.from_numpy(prob['theta0']), torch.from_numpy(test['X']))
    ref = np.stack([RP.forward(spec, RP.params(spec, t, prob['emb'], prob['pos']), test['x'])['logits'] for t in prob['theta0']])
    _assert_close('attn_pre', out, ref)


@pytest.mark.parametrize('F,hs,task', [(5, (64, 64, 64, 2), 'regr'), (8, (32, 32, 7), 'classification')])
def test_log_prob_of_the_outputs_is_pointwise_loglik(F, hs, task):
    from mile_amd import metrics as M
    ospec = O.ModelSpec(F, hs, task=task)
    prob = O.synthetic_problem(ospec, 64, 4, seed=5)              # (small weights: log-probabilities of order 1..100)
    test = O.synthetic_problem(ospec, 301, 1, seed=6)
    eng = _fcn_engine(ospec, prob, 'mfma_w64_bf16x3' if task == 'regr' else 'mfma_narrow_f32')
    th, X, y = torch.from_numpy(prob['theta0'].reshape(2, 2, -1)), torch.from_numpy(test['X']), torch.from_numpy(test['y'])
    raw = eng.predict(th, X)
    assert raw.shape == (2, 2, 301, hs[-1])                      # leading axes of theta are kept
    pw = eng.pointwise_loglik(th, X, y)
    mine = M.pointwise_lppd(raw.double(), y.to(DEV), task)
    _assert_close('log_prob', mine, pw.cpu().numpy().astype(np.float64))


def test_more_samples_than_one_grid_holds():
    """S = 70 000 > 65 535 (gridDim.y): the launch is walked in chunks, every row of every sample is written."""
    ospec = O.ModelSpec(5, (16, 16, 2))
    S, N = 70000, 7
    prob = O.synthetic_problem(ospec, 32, 1, seed=8)
    rng = np.random.default_rng(0)
    theta = (0.3 * rng.standard_normal((S, ospec.n_params))).astype(np.float32)
    X = rng.standard_normal((N, 5)).astype(np.float32)
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    out = eng.predict(torch.from_numpy(theta), torch.from_numpy(X))
    torch.cuda.synchronize()
    assert out.shape == (S, N, 2)
    _assert_close('S=70000 mfma_narrow_f32', out, O.mlp_forward(ospec, theta.astype(np.float64), X.astype(np.float64)))


def test_more_samples_than_one_grid_holds_w64():
    ospec = O.ModelSpec(5, (64, 2))
    S, N = 70000, 7
    prob = O.synthetic_problem(ospec, 32, 1, seed=8)
    rng = np.random.default_rng(1)
    theta = (0.3 * rng.standard_normal((S, ospec.n_params))).astype(np.float32)
    X = rng.standard_normal((N, 5)).astype(np.float32)
    eng = _fcn_engine(ospec, prob, 'mfma_w64')
    out = eng.predict(torch.from_numpy(theta), torch.from_numpy(X))
    torch.cuda.synchronize()
    _assert_close('S=70000 mfma_w64', out, O.mlp_forward(ospec, theta.astype(np.float64), X.astype(np.float64)))


def _loglik_beyond_one_grid(kernel, hs, seed):
    """pointwise_loglik for S = 70 000 > 65 535 (gridDim.y): the library's forward driver walks S in chunks for the
    log-likelihood launches as for the raw outputs; the samples on either side of the seam are checked on their own."""
    ospec = O.ModelSpec(5, hs)
    S, N = 70000, 7
    prob = O.synthetic_problem(ospec, 32, 1, seed=8)
    rng = np.random.default_rng(seed)
    theta = (0.1 * rng.standard_normal((S, ospec.n_params))).astype(np.float32)
    X = rng.standard_normal((N, 5)).astype(np.float32)
    y = rng.standard_normal(N).astype(np.float32)
    eng = _fcn_engine(ospec, prob, kernel)
    out = eng.pointwise_loglik(torch.from_numpy(theta), torch.from_numpy(X), torch.from_numpy(y))
    torch.cuda.synchronize()
    assert out.shape == (S, N)
    ref = O.pointwise_loglik_raw(ospec, O.mlp_forward(ospec, theta.astype(np.float64), X.astype(np.float64)), y.astype(np.float64))[0]
    assert np.isfinite(ref).all()
    _assert_close(f'loglik S=70000 {kernel}', out, ref)
    for row in (65534, 65535, 65536):
        _assert_close(f'loglik S=70000 {kernel} sample {row}', out[row], ref[row])


def test_more_samples_than_one_grid_holds_loglik():
    _loglik_beyond_one_grid('mfma_narrow_f32', (16, 16, 2), 0)


def test_more_samples_than_one_grid_holds_loglik_w64():
    _loglik_beyond_one_grid('mfma_w64', (64, 2), 1)


@pytest.mark.parametrize('kernel,hs', [('mfma_narrow_f32', (16, 16, 2)), ('mfma_w64_bf16x3', (64, 64, 2)), ('gemm_f32', (128, 96, 2))])
def test_nan_passes_through(kernel, hs):
    ospec = O.ModelSpec(5, hs)
    prob = O.synthetic_problem(ospec, 64, 5, seed=3)
    theta = prob['theta0'].copy()
    theta[2, O.param_slices(ospec)[-1]['bias'][0]] = np.nan      # the output layer's bias of mu: no activation can absorb it
    eng = _fcn_engine(ospec, prob, kernel)
    out = eng.predict(torch.from_numpy(theta), torch.from_numpy(prob['X'])).cpu()
    assert torch.isnan(out[2]).any(dim=-1).all()                 # every row of that sample
    assert torch.isfinite(out[[0, 1, 3, 4]]).all()               # and of no other


def _run(args, timeout=600):
    r = subprocess.run([sys.executable] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def _reload(exp, split):
    """What evaluate.py loads: spec, samples [C, S, d], the split and an engine on the training rows."""
    from mile_amd.callbacks import load_samples_from_dir
    from mile_amd.config import Config
    from mile_amd.trainer import BDETrainer
    cfg = Config.from_file(exp / 'config.yaml').replace(logging=False)
    tr = BDETrainer.__new__(BDETrainer)
    tr.build_model(cfg)
    samples = load_samples_from_dir(exp / cfg.training.sampler._dir_name, tr.prob_model.spec)
    x = np.ascontiguousarray(getattr(tr.loader, f'{split}_x')).reshape(len(getattr(tr.loader, f'{split}_x')), -1)
    y = np.ascontiguousarray(getattr(tr.loader, f'{split}_y'))
    eng = tr.prob_model.engine(torch.from_numpy(np.ascontiguousarray(tr.loader.train_x).reshape(len(tr.loader.train_x), -1)),
                               torch.from_numpy(np.ascontiguousarray(tr.loader.train_y)), device=DEV)
    return eng, samples, x, y


def test_evaluate_cli_reports_accuracy(tmp_path):
    import yaml
    from mile_amd import metrics as M
    cfg = yaml.safe_load((ROOT / 'experiments' / 'mclmc_lenetti_mnist.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['experiment_name'] = 'lenetti_small'
    cfg['data']['path'] = '400x1x12x12'
    cfg['data']['datapoint_limit'] = 400
    cfg['training']['warmstart'].update(max_epochs=3, patience=2)
    cfg['training']['sampler'].update(warmup_steps=30, n_samples=20, n_chains=3, n_thinning=10)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    _run([ROOT / 'train.py', '-c', tmp_path / 'cfg.yaml', '-d', '1'])
    exp = tmp_path / 'lenetti_small'
    _run([ROOT / 'evaluate.py', '-e', exp, '--split', 'valid'])
    m = json.loads((exp / 'metrics.json').read_text())
    assert 0.0 <= m['acc'] <= 1.0
    assert len(m['per_chain_acc']) == m['n_chains'] == 3 and all(0.0 <= a <= 1.0 for a in m['per_chain_acc'])
    assert m['per_chain_acc_median'] == pytest.approx(float(np.median(m['per_chain_acc'])), abs=1e-12)
    assert np.isfinite(m['lppd'])                                 # the existing keys are still there
    # the same draws, here: chain by chain from one generator seeded --seed (42), mode over (chain, sample)
    eng, samples, x, y = _reload(exp, 'valid')
    gen = torch.Generator(device=DEV).manual_seed(42)
    xt = torch.from_numpy(x).to(DEV)
    draws = torch.stack([M.sample_from_predictions(eng.predict(torch.from_numpy(samples[c]), xt), 'classification', gen)
                         for c in range(samples.shape[0])])
    K = eng.spec.hidden_structure[-1]
    assert m['acc'] == pytest.approx(float(M.accuracy(draws, torch.from_numpy(y), K)), abs=1e-12)
    for c in range(3):
        assert m['per_chain_acc'][c] == pytest.approx(float(M.accuracy(draws[c], torch.from_numpy(y), K)), abs=1e-12)


def test_evaluate_cli_reports_coverage(tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=30, n_chains=4)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    _run([ROOT / 'train.py', '-c', tmp_path / 'cfg.yaml', '-d', '1'])
    exp = tmp_path / 'smoke_synthetic'
    _run([ROOT / 'evaluate.py', '-e', exp, '--split', 'valid'])
    m = json.loads((exp / 'metrics.json').read_text())
    nominal = [0.5, 0.75, 0.9, 0.95]
    cov = [m[f'coverage_{c}'] for c in nominal]
    assert all(0.0 <= v <= 1.0 for v in cov)
    assert all(a <= b for a, b in zip(cov, cov[1:]))              # nested intervals
    assert m['cal_error'] == pytest.approx(float(np.sqrt(np.mean((np.array(nominal) - np.array(cov)) ** 2))), rel=1e-12)
    assert 'rmse' in m and 'per_chain_rmse' in m                  # the FCN path's own keys
