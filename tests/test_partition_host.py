"""Partition sampling, host side (no GPU): the segment table and partition / merge, the CPU restatement of the partition
target (tests/partition_ref.py) against torch.autograd, the config checks, and the layout of merged sample files."""
import math

import numpy as np
import pytest

from tests import partition_ref as PR

torch = pytest.importorskip('torch')


def _spec(in_features, hidden, **kw):
    from mile_amd import ModelSpec
    return ModelSpec(in_features=in_features, hidden_structure=hidden, **kw)


# ---- layout --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,hidden', [(5, (7, 6, 3, 2)), (3, (4,) * 11 + (2,))])
def test_segments_and_round_trip(oracle, F, hidden):
    from mile_amd import partition as mpart
    spec, ospec = _spec(F, hidden), oracle.ModelSpec(F, hidden)
    n, d = len(hidden), spec.n_params
    segs = mpart.segments(spec)
    assert segs == [(b, e - b) for b, e in PR.segments(ospec)]              # the oracle's param_slices say the same
    # the sampled leaves by name, straight from the leaf table
    want = np.zeros(d, bool)
    for name, off, shape in spec.leaves():
        if name.split('.')[1] in ('layer0', f'layer{n - 1}'):
            want[off:off + int(np.prod(shape))] = True
    idx = mpart.sampled_index(spec)
    assert np.array_equal(np.nonzero(want)[0], idx) and np.all(np.diff(idx) > 0)
    d_s = F * hidden[0] + hidden[0] + hidden[-2] * hidden[-1] + hidden[-1]
    assert mpart.sampled_dim(spec) == d_s == len(idx) and len(segs) == 2
    assert segs[0][0] == 0                                                   # 'layer0' sorts first
    if n == 12:
        # 'layer11' sorts between 'layer10' and 'layer2': the second segment is in the middle of the row, not its tail
        assert segs[1][0] + segs[1][1] < d and spec.layer_order()[:4] == [0, 1, 10, 11]
    else:
        assert segs[1][0] + segs[1][1] == d
    rng = np.random.default_rng(0)
    E = 3
    full = rng.standard_normal((E, d)).astype(np.float32)
    comp = mpart.partition(spec, full)
    assert comp.shape == (E, d_s) and np.array_equal(comp, PR.partition(ospec, full))
    assert np.array_equal(mpart.merge(spec, comp, full), full)
    # new sampled values, several samples at once: frozen coordinates are the frozen rows', bit for bit
    new = rng.standard_normal((4, E, d_s)).astype(np.float32)
    merged = mpart.merge(spec, new, full)
    assert merged.shape == (4, E, d) and merged.dtype == np.float32
    assert np.array_equal(merged[..., idx], new)
    assert np.array_equal(merged[..., ~want], np.broadcast_to(full[:, ~want], (4, E, int((~want).sum()))))
    assert np.array_equal(merged, PR.merge(ospec, new, full))
    # torch tensors take the same path
    mt = mpart.merge(spec, torch.from_numpy(new), torch.from_numpy(full))
    assert torch.equal(mt, torch.from_numpy(merged))
    assert torch.equal(mpart.partition(spec, torch.from_numpy(full)), torch.from_numpy(comp))
    with pytest.raises(ValueError):
        mpart.merge(spec, new[:, :2], full)


def test_two_layer_net_has_no_frozen_layer():
    from mile_amd import partition as mpart
    spec = _spec(4, (6, 2))
    assert mpart.segments(spec) == [(0, spec.n_params)] and mpart.sampled_dim(spec) == spec.n_params


def test_partition_is_for_the_fcn_only():
    from mile_amd import partition as mpart
    from mile_amd.spec import LeNettiSpec
    with pytest.raises(ValueError, match='FCN only'):
        mpart.segments(LeNettiSpec(channels=1, height=8, width=8, out_dim=3))


# ---- the CPU restatement of the target ----------------------------------------------------------------------------------------
def _torch_partition_logp(ospec, compact, frozen, X, y):
    """log_prior(compact) + log_likelihood(net(merge(compact, frozen))) with torch, fp64, written independently of the oracle."""
    idx = torch.from_numpy(PR.index(ospec))
    full = frozen.clone()
    full = full.index_put((torch.arange(full.shape[0])[:, None], idx[None]), compact)
    ents = []
    off = 0
    dims, fin = [], ospec.in_features
    for w in ospec.hidden_structure:
        dims.append((fin, w)); fin = w
    order = sorted(range(len(dims)), key=lambda i: f'layer{i}')
    where = {}
    for li in order:
        i, o = dims[li]
        where[li] = (off, off + o, off + o + i * o); off += o + i * o
    out = []
    for e in range(full.shape[0]):
        h = X
        for li, (i, o) in enumerate(dims):
            b0, k0, k1 = where[li]
            h = h @ full[e, k0:k1].reshape(i, o) + full[e, b0:k0]
            if li + 1 < len(dims):
                h = torch.relu(h) if ospec.activation == 'relu' else torch.tanh(h)
        sig = torch.exp(h[:, 1]).clamp(1e-6, 1e6)
        ll = (-0.5 * ((y - h[:, 0]) / sig) ** 2 - torch.log(sig) - 0.5 * math.log(2 * math.pi)).sum()
        t = (compact[e] - ospec.prior_loc) / ospec.prior_scale
        lp = (-0.5 * t * t - math.log(ospec.prior_scale) - 0.5 * math.log(2 * math.pi)).sum()
        out.append(ll + lp)
    return torch.stack(out)


def test_partition_ref_matches_autograd(oracle):
    ospec = oracle.ModelSpec(3, (4, 4, 2), activation='tanh', prior='Normal', prior_loc=0.1, prior_scale=0.7)
    E, N = 3, 25
    prob = oracle.synthetic_problem(ospec, N, E, seed=4, theta_scale=0.5)
    rng = np.random.default_rng(1)
    frozen = prob['theta0'].astype(np.float64)                       # differs per chain
    compact = PR.partition(ospec, frozen) + 0.3 * rng.standard_normal((E, len(PR.index(ospec))))
    f = PR.logdensity_and_grad(ospec, frozen, prob['X'], prob['y'])
    logp, grad = f(compact)
    assert grad.shape == compact.shape == (E, 3 * 4 + 4 + 4 * 2 + 2)
    c = torch.from_numpy(compact).requires_grad_(True)
    lt = _torch_partition_logp(ospec, c, torch.from_numpy(frozen), torch.from_numpy(prob['X'].astype(np.float64)),
                               torch.from_numpy(prob['y'].astype(np.float64)))
    lt.sum().backward()
    assert np.abs(logp - lt.detach().numpy()).max() < 1e-10 * np.abs(logp).max()
    assert np.abs(grad - c.grad.numpy()).max() < 1e-10 * np.abs(grad).max()


@pytest.mark.parametrize('prior', ['Normal', 'Laplace'])
def test_frozen_prior_does_not_leak_in(oracle, prior):
    """The partition gradient is the full posterior gradient on the segments (a sampled coordinate's prior term is its own),
    the log-density is the full one minus exactly the frozen coordinates' prior, and moving a frozen coordinate's PRIOR
    (scale) term alone -- same likelihood -- cannot change either: checked by shifting the frozen values' prior contribution."""
    ospec = oracle.ModelSpec(5, (6, 5, 4, 2), prior=prior, prior_loc=0.0, prior_scale=0.5)
    E, N = 2, 30
    prob = oracle.synthetic_problem(ospec, N, E, seed=9, theta_scale=0.4)
    frozen = prob['theta0'].astype(np.float64)
    idx = PR.index(ospec)
    hidden = np.setdiff1d(np.arange(ospec.n_params), idx)
    compact = PR.partition(ospec, frozen) * 1.1
    logp, grad = PR.logdensity_and_grad(ospec, frozen, prob['X'], prob['y'])(compact)
    full = PR.merge(ospec, compact, frozen)
    lp_full, g_full = oracle.logpost_and_grad(ospec, full, prob['X'].astype(np.float64), prob['y'].astype(np.float64))
    assert np.array_equal(grad, g_full[:, idx])
    lp_hidden, gp_hidden = oracle.log_prior(ospec, full[:, hidden])
    assert np.abs(lp_hidden).min() > 1.0                                       # a leak would be visible
    assert np.abs((lp_full - logp) - lp_hidden).max() < 1e-9 * np.abs(lp_full).max()
    # likelihood-only statement: log-density minus the sampled coordinates' prior is the likelihood of the merged net
    out = oracle.mlp_forward(ospec, full, prob['X'].astype(np.float64))
    ll, _ = oracle.pointwise_loglik(ospec, out, prob['y'].astype(np.float64))
    lp_s, _ = oracle.log_prior(ospec, compact)
    assert np.abs(logp - (ll.sum(axis=-1) + lp_s)).max() < 1e-9 * np.abs(logp).max()


def test_tuner_step_size_depends_on_the_dimension(oracle):
    """What the GPU tuner test relies on: after a step whose energy change is resolved, the predictor's step size with
    dim = d_s and with dim = d_full differ by far more than the 1e-3 the device is held to (xi ~ dE^2 / dim: a factor
    (d_full / d_s)^(1/6) on the first step)."""
    ospec = oracle.ModelSpec(8, (16,) * 8 + (2,))
    d_full, d_s = ospec.n_params, len(PR.index(ospec))
    assert (d_full, d_s) == (2082, 178)
    f32 = np.float32
    dE = np.array([0.3, -2.0, 0.05], f32)
    eps = np.full(3, 0.01, f32)
    out = {}
    for dim in (d_s, d_full):
        ad = oracle.AdaptiveState.fresh(3, d_s, f32)
        ad.step_size_max = np.nan_to_num(ad.step_size_max)
        out[dim], _, _ = oracle.predictor_update(dE, eps, ad, dim=dim, var=0.5, trust_in_estimate=1.5, decay=f32(99 / 101))
    ratio = out[d_full] / out[d_s]
    assert np.all(np.abs(ratio - 1) > 0.3), ratio
    assert np.allclose(ratio, (d_full / d_s) ** (1 / 6), rtol=1e-3)


# ---- config -------------------------------------------------------------------------------------------------------------------
def _raw():
    import yaml
    from pathlib import Path
    with open(Path(__file__).resolve().parents[1] / 'experiments' / 'mclmc_partition_synthetic.yaml') as f:
        return yaml.safe_load(f)


def test_partition_yaml_is_the_reference_net():
    from mile_amd.config import Config
    cfg = Config.from_dict(_raw())
    assert cfg.training.sampler.partition_sampling is True and cfg.training.sampler.name == 'mclmc'
    assert list(cfg.model.hidden_structure) == [16] * 8 + [2] and cfg.n_chains == 12
    assert cfg.data.source == 'synthetic' and cfg.data.path.endswith('x8')


def test_config_refuses_what_is_not_built():
    from mile_amd.config import Config, ConfigError
    assert issubclass(ConfigError, ValueError)
    d = _raw()
    d['training']['sampler']['name'] = 'nuts'
    with pytest.raises(ValueError, match='nuts is not built yet'):
        Config.from_dict(d)
    d = _raw()
    d['training']['warmstart']['partition_warmstart'] = True
    with pytest.raises(ValueError, match='partition_warmstart is not built'):
        Config.from_dict(d)
    d = _raw()
    d['data'] = dict(d['data'], data_type='image', path='64x1x12x12', task='class')
    d['model'] = {'model': 'LeNetti', 'activation': 'relu', 'out_dim': 3}
    with pytest.raises(ValueError, match='partition_sampling samples the first and the last Dense layer of an FCN'):
        Config.from_dict(d)
    # the same three configurations without the flag are fine, so it is the flag that is refused
    for mut in (lambda d: d['training']['sampler'].update(name='nuts', partition_sampling=False),
                lambda d: d['training']['sampler'].update(partition_sampling=False)):
        d = _raw()
        mut(d)
        Config.from_dict(d)


def test_two_layer_net_with_the_flag_is_accepted():
    from mile_amd.config import Config
    d = _raw()
    d['model']['hidden_structure'] = [16, 2]
    cfg = Config.from_dict(d)
    assert cfg.training.sampler.partition_sampling is True


# ---- sample files ---------------------------------------------------------------------------------------------------------------
def test_merged_sample_files_have_the_layout_of_a_full_run(tmp_path):
    from mile_amd import partition as mpart
    from mile_amd.sample_writer import write_chain_samples
    spec = _spec(3, (4,) * 11 + (2,))
    leaves = [(n, o, tuple(sh)) for n, o, sh in spec.leaves()]
    rng = np.random.default_rng(3)
    E, d = 2, spec.n_params
    frozen = rng.standard_normal((E, d)).astype(np.float32)
    full_run = rng.standard_normal((3, E, d)).astype(np.float32)
    compact = rng.standard_normal((3, E, mpart.sampled_dim(spec))).astype(np.float32)
    merged = mpart.merge(spec, compact, frozen)
    for e in range(E):
        write_chain_samples(leaves, np.ascontiguousarray(full_run[:, e]), str(tmp_path / 'full'), e, [0, 10, 20])
        write_chain_samples(leaves, np.ascontiguousarray(merged[:, e]), str(tmp_path / 'part'), e, [0, 10, 20])
    for e in range(E):
        for n in (0, 10, 20):
            a = np.load(tmp_path / 'full' / str(e) / f'sample_{n}.npz')
            b = np.load(tmp_path / 'part' / str(e) / f'sample_{n}.npz')
            assert a.files == b.files and len(b.files) == 24
            for k in b.files:
                assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype == np.float32
                off, shape = next((o, sh) for nme, o, sh in leaves if nme == k)
                src = frozen[e, off:off + int(np.prod(shape))].reshape(shape)
                if k.split('.')[1] in ('layer0', 'layer11'):
                    assert not np.array_equal(b[k], src)
                else:
                    assert np.array_equal(b[k], src)                        # frozen leaves: the warm-start member, bit for bit
