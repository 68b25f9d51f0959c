"""Host side of the LeNetti target (no GPU): the fp64 restatement against torch autograd, the parameter layout, the config
surface and the geometry checks."""
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip('torch')

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope='module')
def R():
    from tests import lenetti_ref
    return lenetti_ref


def _torch_logpost(ospec, theta, X, y):
    """The same net through torch fp64 autograd: F.conv2d(padding=2) on NCHW, flattened in NHWC order (one channel)."""
    import torch.nn.functional as F
    th = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    x = torch.tensor(X, dtype=torch.float64)
    act = {'relu': torch.relu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}[ospec.activation]
    lps = []
    for e in range(th.shape[0]):
        p = {n: th[e, o:o + int(np.prod(sh))].reshape(sh) for n, o, sh in ospec.leaves()}
        w = p['core.conv1.kernel'].permute(3, 2, 0, 1)                       # [kh, kw, in, out] -> [out, in, kh, kw]
        a = act(F.conv2d(x, w, p['core.conv1.bias'], padding=2))              # [N, 1, H+2, W+2]
        h = a.permute(0, 2, 3, 1).reshape(x.shape[0], -1)                    # NHWC flatten
        for name in ('fc1', 'fc2', 'fc3'):
            h = act(h @ p[f'core.{name}.kernel'] + p[f'core.{name}.bias'])
        out = h @ p['core.fc4.kernel'] + p['core.fc4.bias']
        if ospec.task == 'regr':
            sig = torch.clamp(torch.exp(out[:, 1]), 1e-6, 1e6)
            ll = torch.distributions.Normal(out[:, 0], sig).log_prob(torch.tensor(y, dtype=torch.float64)).sum()
        else:
            ll = torch.log_softmax(out, dim=-1)[torch.arange(x.shape[0]), torch.tensor(y, dtype=torch.long)].sum()
        t = (th[e] - ospec.prior_loc) / ospec.prior_scale
        if ospec.prior == 'Normal':
            lp = (-0.5 * t * t - np.log(ospec.prior_scale) - 0.5 * np.log(2 * np.pi)).sum()
        else:
            lp = (-t.abs() - np.log(2 * ospec.prior_scale)).sum()
        lps.append(ll + lp)
    tot = torch.stack(lps)
    tot.sum().backward()
    return tot.detach().numpy(), th.grad.numpy()


@pytest.mark.parametrize('C,H,W,K,act,task,prior', [
    (1, 6, 7, 10, 'relu', 'classification', 'Normal'),
    (3, 5, 4, 4, 'sigmoid', 'classification', 'Normal'),
    (2, 4, 6, 2, 'tanh', 'regr', 'Laplace'),
])
def test_restatement_matches_torch_autograd(R, C, H, W, K, act, task, prior):
    ospec = R.LeNettiSpec(C, H, W, K, activation=act, task=task, prior=prior, prior_scale=0.7 if prior == 'Laplace' else 1.0)
    prob = R.synthetic_problem(ospec, 9, 2, seed=1)
    th = prob['theta0'].astype(np.float64)
    lp, g = R.logpost_and_grad(ospec, th, prob['X'], prob['y'])
    lp_t, g_t = _torch_logpost(ospec, th, prob['X'], prob['y'])
    np.testing.assert_allclose(lp, lp_t, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(g, g_t, rtol=1e-10, atol=1e-10)


def test_flatten_order_one_hot(R):
    """One non-zero conv-output pixel (h, w), selected by fc1 row h*(W+2) + w: the output moves only through that row."""
    ospec = R.LeNettiSpec(1, 3, 4, 2, activation='relu')
    lv = {n: (o, sh) for n, o, sh in ospec.leaves()}
    theta = np.zeros((1, ospec.n_params))
    o, _ = lv['core.conv1.kernel']
    theta[0, o + 4] = 1.0                                   # centre tap (kh = 1, kw = 1): out(y, x) = in(y - 1, x - 1)
    X = np.zeros((1, 1, 3, 4))
    X[0, 0, 1, 2] = 2.0                                     # -> the conv output at (h, w) = (2, 3) is 2, every other 0
    idx = 2 * (4 + 2) + 3
    o1, _ = lv['core.fc1.kernel']
    for p in range(ospec.pixels):
        th = theta.copy()
        th[0, o1 + p * 8] = 1.0                              # fc1 unit 0 reads pixel p only
        for name in ('fc2', 'fc3'):                          # unit 0 -> unit 0
            th[0, lv[f'core.{name}.kernel'][0]] = 1.0
        th[0, lv['core.fc4.kernel'][0]] = 1.0                # output 0 = unit 0
        out = R.forward(ospec, th, X)
        assert out[0, 0, 0] == (2.0 if p == idx else 0.0), p


def test_spec_layout_matches_the_issue_figures(R):
    from mile_amd import LeNettiSpec
    from mile_amd.tree import ravel_tree, unravel_tree
    for (C, H, W, K), d in (((1, 28, 28, 10), 7452), ((3, 32, 32, 10), 9518)):
        sp, osp = LeNettiSpec(C, H, W, K), R.LeNettiSpec(C, H, W, K)
        P = (H + 2) * (W + 2)
        assert sp.n_params == osp.n_params == d == (1 + 9 * C) + (8 + 8 * P) + 72 + 72 + (K + 8 * K)
        assert [(n, o, tuple(s)) for n, o, s in sp.leaves()] == [(n, o, tuple(s)) for n, o, s in osp.leaves()]
        assert sp.in_features == C * H * W and sp.pixels == P and sp.hidden_structure == (K,)
    sp = LeNettiSpec(1, 28, 28, 10)
    offs = {n: o for n, o, _ in sp.leaves()}
    assert offs == {'core.conv1.bias': 0, 'core.conv1.kernel': 1, 'core.fc1.bias': 10, 'core.fc1.kernel': 18,
                    'core.fc2.bias': 7218, 'core.fc2.kernel': 7226, 'core.fc3.bias': 7290, 'core.fc3.kernel': 7298,
                    'core.fc4.bias': 7362, 'core.fc4.kernel': 7372}
    flat = torch.arange(2 * sp.n_params, dtype=torch.float32).reshape(2, -1)
    tree = unravel_tree(sp, flat)
    assert list(tree) == ['core'] and list(tree['core']) == ['conv1', 'fc1', 'fc2', 'fc3', 'fc4']
    assert tree['core']['conv1']['kernel'].shape == (2, 3, 3, 1, 1) and tree['core']['fc1']['kernel'].shape == (2, 900, 8)
    assert torch.equal(ravel_tree(sp, tree), flat)


def test_yaml_and_reference_model_block_parse():
    import yaml
    from mile_amd.config import Config, LeNettiConfig, _model_config
    cfg = Config.from_file(ROOT / 'experiments' / 'mclmc_lenetti_mnist.yaml')
    assert isinstance(cfg.model, LeNettiConfig) and cfg.model.activation == 'relu' and cfg.model.out_dim == 10
    assert cfg.n_chains == 10 and cfg.rng == 42 and cfg.data.data_type == 'image' and cfg.data.path == '60000x1x28x28'
    assert round(60000 * cfg.data.train_split) == 48000
    s = cfg.training.sampler
    assert (s.name, s.warmup_steps, s.n_samples, s.n_thinning, s.step_size_init) == ('mclmc', 50000, 10000, 100, 0.001)
    assert cfg.training.warmstart.include and cfg.training.warmstart.batch_size == 32
    # the reference YAML's model block, as a dict
    block = yaml.safe_load("model:\n  model: LeNetti\n  activation: 'relu'\n  out_dim: 10\n  use_bias: true\n")['model']
    assert _model_config(block) is LeNettiConfig and LeNettiConfig(**block).activation == 'relu'
    assert LeNettiConfig().activation == 'sigmoid'           # the reference's default
    from mile_amd.config import ConfigError
    with pytest.raises(ConfigError):
        LeNettiConfig(activation='gelu')
    assert s.grad_kernel == 'auto'
    d = cfg.to_dict()
    d['training']['sampler']['grad_kernel'] = 'lenetti_f32'
    assert Config.from_dict(d).training.sampler.grad_kernel == 'lenetti_f32'


def test_init_scales_follow_fan_in(tmp_path):
    import yaml
    from mile_amd.config import Config
    from mile_amd.trainer import BDETrainer
    cfg = yaml.safe_load((ROOT / 'experiments' / 'mclmc_lenetti_mnist.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['data']['path'] = '64x3x10x12'
    cfg['data']['datapoint_limit'] = 64
    (tmp_path / 'c.yaml').write_text(yaml.safe_dump(cfg))
    tr = BDETrainer(Config.from_file(tmp_path / 'c.yaml'))
    sp = tr.prob_model.spec
    assert type(sp).__name__ == 'LeNettiSpec' and (sp.channels, sp.height, sp.width) == (3, 10, 12)
    w = tr.init_module_params(list(range(400)))
    lv = {n: (o, sh) for n, o, sh in sp.leaves()}
    for name, fan_in in (('core.conv1.kernel', 27), ('core.fc1.kernel', 12 * 14), ('core.fc2.kernel', 8), ('core.fc4.kernel', 8)):
        o, sh = lv[name]
        v = w[:, o:o + int(np.prod(sh))]
        assert abs(v.std() * np.sqrt(fan_in) - 1.0) < 0.08, name
        assert np.abs(v).max() <= 2.0 / np.sqrt(fan_in) / 0.87962566103423978 + 1e-6
    o, sh = lv['core.fc1.bias']
    assert not w[:, o:o + 8].any()


def test_unsupported_geometries_are_refused():
    from mile_amd import LeNettiSpec
    LeNettiSpec(1, 1, 1, 3)                                  # smallest image
    LeNettiSpec(4, 40, 40, 16)                               # 42 * 42 = 1764 pixels, 4 channels, 16 outputs
    with pytest.raises(NotImplementedError, match='channels'):
        LeNettiSpec(5, 10, 10, 10)
    with pytest.raises(NotImplementedError, match='2048'):
        LeNettiSpec(1, 44, 44, 10)                           # 46 * 46 = 2116 pixels
    with pytest.raises(NotImplementedError, match='out_dim'):
        LeNettiSpec(1, 28, 28, 17)
    with pytest.raises(ValueError, match='out_dim == 2'):
        LeNettiSpec(1, 28, 28, 3, task='regr')
    with pytest.raises(ValueError):
        LeNettiSpec(1, 0, 28, 10)
    with pytest.raises(NotImplementedError):
        LeNettiSpec(1, 28, 28, 10, use_bias=False)
    from mile_amd.probabilistic import ProbabilisticModel
    from mile_amd.priors import Prior
    pm = ProbabilisticModel(LeNettiSpec(1, 28, 28, 10), prior=Prior.from_name('Normal', loc=0.0, scale=0.5), task='class')
    assert type(pm.spec).__name__ == 'LeNettiSpec' and pm.spec.prior_scale == 0.5 and pm.n_params == 7452
