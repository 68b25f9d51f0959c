"""CPU tests of the host side: C-ABI surface, layouts, config, I/O formats, tuner arithmetic,
diagnostics, LPPD and the world_size-2 (gloo) sharding path.  No GPU compute."""
import math
import os
import re
import sys
from functools import partial
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import mclmc_oracle as O

ROOT = Path(__file__).resolve().parents[1]


# ---------------------------------------------------------------- C ABI -----------------
def test_library_exports_every_declared_symbol():
    from mile_amd import _lib
    from mile_amd._build import build_library
    build_library()                                   # hipcc cross-compiles without a GPU
    lib = _lib.load_library()
    header = (ROOT / 'include' / 'mile_hip.h').read_text()
    declared = set(re.findall(r'\b(mile_[a-z_]+)\s*\(', header))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.mile_abi_version() == _lib.ABI_VERSION
    # struct layouts agree with the header's field order
    for cls, name in ((_lib.StepArgsC, 'mile_step_args'), (_lib.TuneArgsC, 'mile_tune_args'),
                      (_lib.StateC, 'mile_state'), (_lib.ModelSpecC, 'mile_model_spec')):
        body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), header, re.S).group(1), flags=re.S)
        fields = re.findall(r'(?:const\s+)?\w+\s*\*?\s*(\w+)(?:\[\w+\])?\s*;', body)
        assert [f[0] for f in cls._fields_] == fields, name


def test_host_calls_that_need_no_gpu():
    """create / param_count / param_offsets / destroy and argument validation run on the host."""
    import ctypes as C
    from mile_amd import _lib
    lib = _lib.load_library()
    cs = _lib.ModelSpecC()
    cs.in_features, cs.n_layers = 5, 12
    for i in range(12):
        cs.widths[i] = 4
    cs.widths[11] = 2
    cs.activation, cs.task, cs.prior, cs.prior_loc, cs.prior_scale, cs.use_bias = 0, 0, 0, 0.0, 1.0, 1
    h = C.c_void_p()
    assert lib.mile_create(C.byref(cs), 0, C.byref(h)) == 0
    spec = O.ModelSpec(5, (4,) * 11 + (2,))
    assert lib.mile_param_count(h) == spec.n_params
    for li, ent in enumerate(O.param_slices(spec)):      # same ravel order incl. layer10 < layer2
        b, k = C.c_int64(), C.c_int64()
        assert lib.mile_param_offsets(h, li, C.byref(b), C.byref(k)) == 0
        assert (b.value, k.value) == (ent['bias'][0], ent['kernel'][0])
    assert lib.mile_destroy(h) == 0
    cs.widths[11] = 3                                     # regression needs width 2
    assert lib.mile_create(C.byref(cs), 0, C.byref(h)) == -1
    assert b'width 2' in lib.mile_last_error()
    cs.widths[11] = 2
    cs.prior_scale = 0.0
    assert lib.mile_create(C.byref(cs), 0, C.byref(h)) == -1


def _fcn_cspec(F, widths, act=0, task=0):
    from mile_amd import _lib
    cs = _lib.ModelSpecC()
    cs.in_features, cs.n_layers = F, len(widths)
    for i, w in enumerate(widths):
        cs.widths[i] = w
    cs.activation, cs.task, cs.prior, cs.prior_loc, cs.prior_scale, cs.use_bias = act, task, 0, 0.0, 1.0, 1
    return cs


def _image_cspec(model, c, h, w, k):
    cs = _fcn_cspec(c * h * w, (k,), task=1)
    cs.model, cs.img_c, cs.img_h, cs.img_w = model, c, h, w
    return cs


def _attn_cspec():
    cs = _fcn_cspec(16, (3,), task=1)
    cs.model, cs.vocab_size, cs.ctx_len, cs.emb_size, cs.n_heads, cs.qkv_dim = 3, 50, 16, 16, 2, 16
    return cs


# spec -> (AUTO, AUTO under MILE_NO_NARROW, the ids mile_set_grad_kernel accepts).  Ids: 1 generic, 2 mfma_w64,
# 3 mfma_w128_bf16, 4 gemm_f32, 5 lenet_f32, 6 mfma_w64_bf16x3, 7 mfma_wide_bf16x3, 8 mfma_wide_bf16, 9 lenet_bf16,
# 10 mfma_narrow_f32, 11 lenetti_f32, 12 attn_f32
KERNEL_CHOICE = {
    'w64_3': (lambda: _fcn_cspec(5, (64, 64, 64, 2)), 6, 6, {1, 2, 4, 6, 7, 8, 10}),
    'w64_1': (lambda: _fcn_cspec(5, (64, 2)), 2, 2, {1, 2, 4, 7, 8, 10}),
    'w64_f17': (lambda: _fcn_cspec(17, (64, 64, 2)), 10, 1, {1, 4, 7, 8, 10}),          # refused by W64: F > 16
    'w128': (lambda: _fcn_cspec(5, (128, 128, 2)), 7, 7, {1, 3, 4, 7, 8}),
    'w128_cls': (lambda: _fcn_cspec(5, (128, 128, 3), task=1), 7, 7, {1, 4, 7, 8}),     # refused by W128: not regression
    'narrow': (lambda: _fcn_cspec(5, (16, 16, 2), act=1), 10, 1, {1, 4, 7, 8, 10}),
    'narrow_lds': (lambda: _fcn_cspec(5, (48, 48, 2)), 10, 1, {1, 4, 7, 8, 10}),
    'deep32': (lambda: _fcn_cspec(5, (32,) * 4 + (2,)), 1, 1, {1, 4, 7, 8}),           # refused by NARROW: 4 layers > 16 wide
    'wide': (lambda: _fcn_cspec(5, (256, 256, 2)), 7, 7, {1, 4, 7, 8}),
    'generic': (lambda: _fcn_cspec(80, (32, 2)), 1, 1, {1, 4, 7, 8}),
    'lenet_c1': (lambda: _image_cspec(1, 1, 28, 28, 10), 5, 5, {5, 9}),
    'lenet_c5': (lambda: _image_cspec(1, 5, 16, 16, 10), 5, 5, {5}),
    'lenetti': (lambda: _image_cspec(2, 1, 8, 8, 3), 11, 11, {11}),
    'attn': (lambda: _attn_cspec(), 12, 12, {12}),
}


@pytest.mark.parametrize('name', sorted(KERNEL_CHOICE))
def test_grad_kernel_choice_matrix(name, monkeypatch):
    """mile_set_grad_kernel accepts exactly the kernels that run the spec (refusing the rest as invalid), and AUTO picks
    by the documented priority, with or without MILE_NO_NARROW.  Host only: no GPU."""
    import ctypes as C
    from mile_amd import _lib
    lib = _lib.load_library()
    make, auto, auto_no_narrow, accepted = KERNEL_CHOICE[name]
    h = C.c_void_p()
    assert lib.mile_create(C.byref(make()), 0, C.byref(h)) == 0, lib.mile_last_error()
    try:
        assert lib.mile_get_grad_kernel(h) == auto
        monkeypatch.setenv('MILE_NO_NARROW', '1')
        assert lib.mile_get_grad_kernel(h) == auto_no_narrow
        monkeypatch.delenv('MILE_NO_NARROW')
        for k in range(1, 13):
            rc = lib.mile_set_grad_kernel(h, k)
            if k in accepted:
                assert rc == 0, (k, lib.mile_last_error())
                assert lib.mile_get_grad_kernel(h) == k
            else:
                assert rc == -1 and lib.mile_last_error(), k
                assert lib.mile_get_grad_kernel(h) == auto     # a refusal leaves the choice as it was
            assert lib.mile_set_grad_kernel(h, 0) == 0
        assert lib.mile_set_grad_kernel(h, 13) == -1 and lib.mile_set_grad_kernel(h, -1) == -1
    finally:
        assert lib.mile_destroy(h) == 0


@pytest.mark.parametrize('model', ['lenet', 'lenetti'])
def test_image_model_param_offsets_follow_leaves(model):
    """mile_param_offsets of the image models (layers conv1, then the Dense layers) against spec.leaves()."""
    import ctypes as C
    from mile_amd import _lib
    from mile_amd.spec import LeNetSpec, LeNettiSpec
    lib = _lib.load_library()
    spec = LeNetSpec(3, 32, 32, 10) if model == 'lenet' else LeNettiSpec(2, 9, 7, 5)
    layers = ['conv1', 'conv2', 'fc1', 'fc2', 'fc3'] if model == 'lenet' else ['conv1', 'fc1', 'fc2', 'fc3', 'fc4']
    h = C.c_void_p()
    cs = _image_cspec(1 if model == 'lenet' else 2, spec.channels, spec.height, spec.width, spec.out_dim)
    assert lib.mile_create(C.byref(cs), 0, C.byref(h)) == 0, lib.mile_last_error()
    assert lib.mile_param_count(h) == spec.n_params
    L = {n: o for n, o, _ in spec.leaves()}
    for li, nm in enumerate(layers):
        b, k = C.c_int64(), C.c_int64()
        assert lib.mile_param_offsets(h, li, C.byref(b), C.byref(k)) == 0
        assert (b.value, k.value) == (L[f'core.{nm}.bias'], L[f'core.{nm}.kernel']), nm
    assert lib.mile_param_offsets(h, len(layers), C.byref(b), C.byref(k)) == -1
    assert lib.mile_destroy(h) == 0


def test_product_path_fails_loudly_without_gpu_or_library(tmp_path):
    from mile_amd import ModelSpec, _lib
    with pytest.raises(_lib.MileHipError):
        _lib.load_library(tmp_path / 'nope.so')
    if not torch.cuda.is_available():
        from mile_amd.engine import Engine
        with pytest.raises(_lib.MileHipError):
            Engine(ModelSpec(5, (8, 2)), torch.zeros(4, 5), torch.zeros(4))


def test_product_never_imports_the_oracle():
    for p in (ROOT / 'mile_amd').rglob('*.py'):
        assert 'oracle' not in re.sub(r'#.*', '', p.read_text()).replace('"""', ''), p
    assert 'oracle' not in (ROOT / 'train.py').read_text()


# ---------------------------------------------------------------- layout / tree ----------
def test_spec_leaves_and_tree_roundtrip():
    from mile_amd import ModelSpec
    from mile_amd.tree import get_flattened_keys, ravel_tree, unravel_tree
    spec = ModelSpec(5, (16, 16, 2))
    ospec = O.ModelSpec(5, (16, 16, 2))
    assert [n for n, _, _ in spec.leaves()] == O.flattened_keys(ospec)
    assert spec.n_params == ospec.n_params == 402
    flat = torch.arange(3 * 402, dtype=torch.float32).reshape(3, 402)
    tree = unravel_tree(spec, flat)
    assert get_flattened_keys(tree) == O.flattened_keys(ospec)
    assert tree['fcn']['layer0']['kernel'].shape == (3, 5, 16)
    assert torch.equal(ravel_tree(spec, tree), flat)
    # same slices as the oracle's unravel
    (W0, b0), *_ = O.unravel(ospec, flat.numpy())
    assert np.array_equal(tree['fcn']['layer0']['kernel'].numpy(), W0) and np.array_equal(tree['fcn']['layer0']['bias'].numpy(), b0)
    big = ModelSpec(3, (4,) * 11 + (2,))
    assert [n for n, _, _ in big.leaves()] == O.flattened_keys(O.ModelSpec(3, (4,) * 11 + (2,)))


def test_prng_key_split_is_deterministic_and_distinct():
    from mile_amd.tree import PRNGKey
    k = PRNGKey(4)
    a, b, c = k.split(3)
    assert (a.seed, b.seed, c.seed) == tuple(x.seed for x in PRNGKey(4).split(3))
    assert len({a.seed, b.seed, c.seed, k.seed}) == 4
    assert k.fold_in(1).seed != k.fold_in(2).seed


# ---------------------------------------------------------------- config ----------------
def test_config_accepts_reference_schema_and_rejects_unknown_keys(tmp_path):
    import yaml
    from mile_amd.config import Config, ConfigError
    cfg = Config.from_file(ROOT / 'experiments' / 'mclmc_airfoil_b1.yaml')
    s = cfg.training.sampler
    assert (s.name, s.warmup_steps, s.n_chains, s.n_samples, s.n_thinning) == ('mclmc', 50000, 16, 10000, 10)
    assert cfg.model.hidden_structure == [64, 64, 64, 2] and s.prior.name == 'StandardNormal'
    assert (s.desired_energy_var_start, s.desired_energy_var_end, s.step_size_init) == (0.5, 0.1, 0.001)
    d = cfg.to_dict()
    d['training']['sampler']['not_a_field'] = 1
    (tmp_path / 'bad.yaml').write_text(yaml.safe_dump(d))
    with pytest.raises(ConfigError, match='unknown field'):
        Config.from_file(tmp_path / 'bad.yaml')
    d = cfg.to_dict()
    del d['data']['path']
    with pytest.raises(ConfigError, match='missing required'):
        Config.from_dict(d)
    # the reference's stock experiment, restated value for value in the repository (only saving_dir / experiment_name
    # differ), parses unchanged
    r = Config.from_file(ROOT / 'experiments' / 'mclmc_airfoil_stock.yaml')
    assert r.n_chains == 12 and r.model.hidden_structure == [16, 16, 2]
    rs = r.training.sampler
    assert (rs.warmup_steps, rs.n_samples, rs.n_thinning, rs.desired_energy_var_start, rs.desired_energy_var_end) == \
        (50000, 10000, 10, 0.5, 0.1)
    assert r.training.warmstart.include and r.rng == 4
    from mile_amd.kernels import KERNELS, WARMUP_KERNELS
    assert s.kernel is KERNELS['mclmc'] and WARMUP_KERNELS == {}


def test_config_grad_kernel_extension_and_all_experiment_yamls_parse():
    from mile_amd.config import Config, ConfigError
    names = {}
    for f in sorted((ROOT / 'experiments').glob('*.yaml')):
        c = Config.from_file(f)
        names[f.name] = c.training.sampler.grad_kernel
    assert names['mclmc_protein_b3.yaml'] == 'mfma_w128_bf16' and names['mclmc_airfoil_b2.yaml'] == 'auto'
    b4 = Config.from_file(ROOT / 'experiments' / 'mclmc_covertype_b4.yaml')
    assert b4.model.hidden_structure == [256, 256, 256, 256, 7] and b4.n_chains == 1024 and b4.data.task == 'class'
    d = b4.to_dict()
    d['training']['sampler']['grad_kernel'] = 'fp8_magic'
    with pytest.raises(ConfigError, match='grad_kernel'):
        Config.from_dict(d)


def test_random_chain_init_follows_flax_dense_defaults(tmp_path):
    """Without warm-start parameters the reference starts chains from module.init (trainer.py:206-228,904-917):
    nn.Dense defaults = lecun_normal kernels (truncated at 2 sigma, variance 1/fan_in), zero biases."""
    import yaml
    from mile_amd.config import Config
    from mile_amd.trainer import BDETrainer
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    (tmp_path / 'c.yaml').write_text(yaml.safe_dump(cfg))
    tr = BDETrainer(Config.from_file(tmp_path / 'c.yaml'))
    w = tr.init_module_params([0, 1, 7])
    assert w.shape == (3, tr.prob_model.spec.n_params) and w.dtype == np.float32
    assert not np.array_equal(w[0], w[1])
    assert np.array_equal(w[2], tr.init_module_params([7])[0])          # stream keyed by the global chain id
    for name, off, shape in tr.prob_model.spec.leaves():
        v = w[:, off:off + int(np.prod(shape))]
        if name.endswith('bias'):
            assert not v.any()
        else:
            sd = math.sqrt(1.0 / shape[0])
            assert abs(v.std() / sd - 1.0) < 0.1, (name, v.std(), sd)
            assert np.abs(v).max() <= 2.0 * sd / 0.87962566103423978 + 1e-6


def test_lenet_spec_config_and_image_loader(tmp_path):
    """Host side of the LeNet target: parameter layout == the oracle's (ravel_pytree order), YAML dispatch on
    `model`, synthetic / npz image loading and splits, flax-style conv initialisation (fan_in = kh*kw*in)."""
    import yaml
    from mile_amd import LeNetSpec
    from mile_amd.config import Config, ConfigError, DataConfig
    from mile_amd.dataset import ImageLoader
    from mile_amd.trainer import BDETrainer
    from mile_amd.tree import ravel_tree, unravel_tree
    from oracle import lenet_oracle as LN
    sp, osp = LeNetSpec(3, 32, 32, 10), LN.LeNetSpec(3, 32, 32, 10)
    assert sp.n_params == osp.n_params == 83126 and sp.in_features == 3072 and sp.flat == 576
    assert [(n, o, tuple(s)) for n, o, s in sp.leaves()] == [(n, o, tuple(s)) for n, o, s in osp.leaves()]
    flat = torch.arange(2 * sp.n_params, dtype=torch.float32).reshape(2, -1)
    tree = unravel_tree(sp, flat)
    assert list(tree) == ['core'] and list(tree['core']) == ['conv1', 'conv2', 'fc1', 'fc2', 'fc3']
    assert tree['core']['conv1']['kernel'].shape == (2, 5, 5, 3, 6)
    assert torch.equal(ravel_tree(sp, tree), flat)
    with pytest.raises(ValueError):
        LeNetSpec(1, 11, 28, 10)                        # (11 // 2 - 4) // 2 == 0
    cfg = Config.from_file(ROOT / 'experiments' / 'mclmc_cifar_lenet_b5.yaml')
    assert type(cfg.model).__name__ == 'LeNetConfig' and cfg.model.out_dim == 10 and cfg.data.data_type == 'image'
    d = cfg.to_dict()
    d['model']['model'] = 'ResNet'
    with pytest.raises(ConfigError, match='Could not find model'):
        Config.from_dict(d)
    dc = DataConfig(path='40x2x12x14', source='synthetic', data_type='image', task='class', normalize=True,
                    train_split=0.5, valid_split=0.25, test_split=0.25)
    ld = ImageLoader(dc, rng=3)
    assert ld.train_x.shape == (20, 2, 12, 14) and ld.valid_x.shape == (10, 2, 12, 14) and ld.test_y.shape == (10,)
    assert ld.train_y.dtype == np.int32 and 0 <= ld.train_y.min() and ld.train_y.max() < 10 and ld.train_x.dtype == np.float32
    np.savez(tmp_path / 'img.npz', x=np.ones((8, 1, 12, 12), np.float32), y=np.arange(8) % 3)
    l2 = ImageLoader(DataConfig(path=str(tmp_path / 'img.npz'), source='local', data_type='image', task='class',
                                train_split=0.5, valid_split=0.25, test_split=0.25), rng=0)
    assert l2.train_x.shape == (4, 1, 12, 12) and len(l2) == 8
    y = yaml.safe_load((ROOT / 'experiments' / 'mclmc_cifar_lenet_b5.yaml').read_text())
    y['saving_dir'] = str(tmp_path)
    y['data']['path'] = '30x3x16x16'
    (tmp_path / 'c.yaml').write_text(yaml.safe_dump(y))
    tr = BDETrainer(Config.from_file(tmp_path / 'c.yaml'))
    assert tr.prob_model.spec.task == 'classification' and tr.prob_model.spec.flat == 64
    w = tr.init_module_params([0])
    for name, off, shape in tr.prob_model.spec.leaves():
        v = w[0, off:off + int(np.prod(shape))]
        if name.endswith('bias'):
            assert not v.any()
        else:
            fan_in = int(np.prod(shape[:-1]))
            assert np.abs(v).max() <= 2.0 * math.sqrt(1.0 / fan_in) / 0.87962566103423978 + 1e-6 and v.std() > 0


def test_warmstart_earlystop_and_adamw_rules():
    """earlystop as trainer.py:920-939; one AdamW step as optax computes it."""
    from mile_amd.warmstart import _Optimizer, earlystop
    losses = torch.tensor([[5.0, 4.0, 4.1, 4.2, 4.3], [5.0, 4.0, 3.9, 4.2, 3.8], [1.0, 2.0, 3.0, 4.0, 5.0]])
    assert earlystop(losses, 3).tolist() == [True, False, True]
    assert earlystop(losses[:, :3], 3).tolist() == [False, False, False]           # not enough history yet
    th = torch.tensor([[1.0, -2.0]]); g = torch.tensor([[0.5, 0.25]])
    opt = _Optimizer('adamw', {'learning_rate': 0.1, 'b1': 0.9, 'b2': 0.999, 'eps': 1e-8, 'weight_decay': 0.01}, th)
    new = opt.step(th, g, torch.tensor([True]))
    # first step: m_hat = g, v_hat = g^2 -> update = lr * (sign(g) + wd * theta)
    assert torch.allclose(new, th - 0.1 * (torch.sign(g) + 0.01 * th), atol=1e-6)
    frozen = opt.step(new, g, torch.tensor([False]))
    assert torch.equal(frozen, new)


def test_train_plan_matches_reference_semantics():
    from mile_amd.sampling import kept_indices
    from mile_amd.trainer import train_plan
    assert [p.tolist() for p in train_plan(12, 4)] == [p.tolist() for p in O.train_plan(12, 4)]
    with pytest.raises(ValueError):
        train_plan(12, 5)
    for n, t in ((10000, 10), (25, 10), (7, 1), (5, 100)):
        assert np.array_equal(kept_indices(n, t), O.kept_indices(n, t))
        assert kept_indices(n, t).dtype == np.int32


# ---------------------------------------------------------------- I/O -------------------
def test_sample_files_have_reference_layout(tmp_path):
    from mile_amd import ModelSpec
    from mile_amd.callbacks import (load_params_batch, load_samples_from_dir, save_flat_sample, save_params,
                                    save_position)
    from mile_amd.tree import unravel_tree
    spec = ModelSpec(5, (16, 16, 2))
    rng = np.random.default_rng(0)
    flat = rng.standard_normal((2, 3, 402)).astype(np.float32)        # [chains, samples, d]
    for c in range(2):
        for k, n in enumerate((0, 10, 20)):
            save_flat_sample(spec, flat[c, k], tmp_path / 'samples', idx=c + 4, n=n)
    f = tmp_path / 'samples' / '4' / 'sample_10.npz'
    assert f.exists()
    with np.load(f) as z:
        assert z.files == ['fcn.layer0.bias', 'fcn.layer0.kernel', 'fcn.layer1.bias', 'fcn.layer1.kernel',
                           'fcn.layer2.bias', 'fcn.layer2.kernel']
        assert z['fcn.layer0.kernel'].shape == (5, 16) and z['fcn.layer0.kernel'].dtype == np.float32
    back = load_samples_from_dir(tmp_path / 'samples', spec)
    assert back.shape == (2, 3, 402) and np.array_equal(back, flat)
    # save_position on a tree writes the identical file
    tree = unravel_tree(spec, torch.from_numpy(flat[0, 1]))
    save_position(tree, tmp_path / 's2', idx=np.int32(4), n=10)
    with np.load(tmp_path / 's2' / '4' / 'sample_10.npz') as z2, np.load(f) as z:
        assert z2.files == z.files and all(np.array_equal(z2[k], z[k]) for k in z.files)
    # warm-start params: sorted by integer suffix, not lexicographically
    for i in (0, 2, 10):
        save_params(tmp_path / 'warmstart', spec, flat[0, 0] + i, i)
    files = [tmp_path / 'warmstart' / f'params_{i}.npz' for i in (10, 2, 0)]
    got = load_params_batch(files, spec)
    assert np.allclose(got[:, 0] - flat[0, 0, 0], [0, 2, 10])
    assert (tmp_path / 'tree').exists()


def test_writer_pool_subprocesses_write_the_same_files(tmp_path):
    from mile_amd import ModelSpec
    from mile_amd.callbacks import load_samples_from_dir, save_flat_sample
    from mile_amd.sample_writer import WriterPool
    spec = ModelSpec(5, (16, 16, 2))
    leaves = [(n, o, tuple(sh)) for n, o, sh in spec.leaves()]
    flat = np.random.default_rng(0).standard_normal((3, 4, 402)).astype(np.float32)
    pool = WriterPool(2)
    for c in range(3):
        pool.submit(leaves, flat[c], str(tmp_path / 'samples'), c + 5, [0, 10, 20, 30])
    assert pool.close() == 12
    assert np.array_equal(load_samples_from_dir(tmp_path / 'samples', spec), flat)
    save_flat_sample(spec, flat[0, 1], tmp_path / 'ref', 5, 10)          # same bytes as the in-process writer
    with np.load(tmp_path / 'ref' / '5' / 'sample_10.npz') as a, np.load(tmp_path / 'samples' / '5' / 'sample_10.npz') as b:
        assert a.files == b.files and all(np.array_equal(a[k], b[k]) for k in a.files)


def test_npz_container_is_what_numpy_writes_and_reads(tmp_path):
    """mile_amd.sample_writer.write_npz (round 3: the per-sample files without numpy's / zipfile's per-member overhead and, by
    default, with STORED deflate blocks -- fp32 samples do not compress) against np.savez_compressed (callbacks.py:42 of the
    reference): same member names in the same order, same .npy payloads bit for bit, deflate method, intact CRCs; np.load
    and zipfile read both alike, at every deflate level."""
    import zipfile
    from mile_amd.sample_writer import write_npz
    rng = np.random.default_rng(0)
    mem = [('fcn.layer0.bias', rng.standard_normal(16).astype(np.float32)),
           ('fcn.layer0.kernel', rng.standard_normal((5, 16)).astype(np.float32)),
           ('labels', np.arange(7, dtype=np.int32)), ('scalar', np.float32(3.5).reshape(())),
           ('empty', np.zeros((0, 3), np.float32)), ('strided', rng.standard_normal((4, 12)).astype(np.float32)[:, ::2])]      # neither C- nor F-contiguous
    np.savez_compressed(tmp_path / 'ref.npz', **dict(mem))
    with zipfile.ZipFile(tmp_path / 'ref.npz') as zr:
        ref_members = {i.filename: zr.read(i.filename) for i in zr.infolist()}
        ref_order = [i.filename for i in zr.infolist()]
    for level in (0, 1, 6):
        f = tmp_path / f'l{level}.npz'
        write_npz(f, mem, level)
        with zipfile.ZipFile(f) as zf:
            assert zf.testzip() is None
            assert [i.filename for i in zf.infolist()] == ref_order
            assert all(i.compress_type == zipfile.ZIP_DEFLATED for i in zf.infolist())
            assert all(zf.read(n) == ref_members[n] for n in ref_order)         # identical .npy bytes (header + data)
        with np.load(f, allow_pickle=False) as z:
            assert z.files == [k for k, _ in mem]
            for k, a in mem:
                assert z[k].dtype == a.dtype and z[k].shape == a.shape and np.array_equal(z[k], a)
    assert (tmp_path / 'l0.npz').stat().st_size < 1.2 * (tmp_path / 'ref.npz').stat().st_size + 1024


def test_tabular_loader_normalises_and_splits(tmp_path):
    from mile_amd.config import DataConfig
    from mile_amd.dataset import TabularLoader
    rng = np.random.default_rng(1)
    data = rng.standard_normal((103, 6)) * 5 + 2
    np.savetxt(tmp_path / 'toy.data', data, delimiter=' ')
    cfg = DataConfig(path=str(tmp_path / 'toy.data'), source='local', data_type='tabular', task='regr',
                     normalize=True, train_split=0.7, valid_split=0.1, test_split=0.2)
    ld = TabularLoader(cfg, rng=4)
    assert len(ld.data_train) == int(103 * 0.7) and len(ld.data_valid) == int(103 * 0.8) - int(103 * 0.7)
    assert ld.train_x.shape == (72, 5) and ld.train_y.shape == (72,)
    assert np.abs(ld.data.mean(axis=0)).max() < 1e-5 and np.abs(ld.data.std(axis=0) - 1).max() < 1e-4
    syn = TabularLoader(DataConfig(path='200x5', source='synthetic', data_type='tabular', task='regr'), rng=0)
    assert syn.train_x.shape == (160, 5)


# ---------------------------------------------------------------- tuner arithmetic -------
def test_predictor_update_and_nan_handling_match_oracle_formulas():
    from mile_amd.engine import IntegratorState
    from mile_amd.warmup import desired_energy_var, handle_nans, predictor_update, streaming_average_update
    for step in (0, 7, 101, 400):
        for start in (0.5, 5.0):
            assert desired_energy_var(step, 101, start, 0.1) == pytest.approx(O.desired_energy_var(step, 101, start, 0.1), rel=1e-12)
    E, d = 5, 30
    rng = np.random.default_rng(2)
    dE = torch.tensor(rng.standard_normal(E), dtype=torch.float64)
    eps = torch.full((E,), 0.01, dtype=torch.float64)
    time, xavg = torch.rand(E, dtype=torch.float64), torch.rand(E, dtype=torch.float64) * 1e10
    # handle_nans has already turned the initial inf into the largest finite float (nan_to_num),
    # which is what keeps `(new > max) * max` from being 0 * inf
    big = float(np.finfo(np.float32).max)
    emax = torch.tensor([big, 0.005, big, 1e-4, big], dtype=torch.float64)
    new, t2, x2 = predictor_update(dE, eps, time, xavg, emax, dim=d, desired_var=0.3, trust_in_estimate=1.5,
                                   decay_rate=99 / 101)
    xi = dE.numpy() ** 2 / (d * 0.3) + 1e-8
    w = np.exp(-0.5 * (np.log(xi) / 9.0) ** 2)
    xr = 99 / 101 * xavg.numpy() + w * xi / 0.01 ** 6
    tr = 99 / 101 * time.numpy() + w
    ref = np.minimum((xr / tr) ** (-1 / 6), emax.numpy())
    assert np.allclose(new.numpy(), ref, rtol=1e-12) and np.allclose(t2.numpy(), tr) and np.allclose(x2.numpy(), xr)
    # handle_nans: chain 1 diverged
    prev = IntegratorState(torch.zeros(2, 4), torch.ones(2, 4), torch.zeros(2), torch.ones(2, 4))
    pos = torch.ones(2, 4)
    pos[1, 2] = float('nan')
    nxt = IntegratorState(pos, 2 * torch.ones(2, 4), torch.tensor([1.0, float('nan')]), 3 * torch.ones(2, 4))
    ok, st, emax2, dE2 = handle_nans(prev, nxt, torch.tensor([0.1, 0.2]), torch.tensor([float('inf')] * 2),
                                     torch.tensor([0.5, float('nan')]))
    assert ok.tolist() == [True, False]
    assert torch.equal(st.position[1], prev.position[1]) and torch.equal(st.position[0], nxt.position[0])
    assert emax2[1].item() == pytest.approx(0.16) and emax2[0].item() > 1e30 and dE2.tolist() == [0.5, 0.0]
    o_ok, o_st, o_emax, o_dE = O.handle_nans(
        O.State(prev.position.numpy(), prev.momentum.numpy(), prev.logdensity.numpy(), prev.logdensity_grad.numpy()),
        O.State(nxt.position.numpy(), nxt.momentum.numpy(), nxt.logdensity.numpy(), nxt.logdensity_grad.numpy()),
        np.array([0.1, 0.2], np.float32), np.array([np.inf, np.inf], np.float32), np.array([0.5, np.nan], np.float32))
    assert o_ok.tolist() == ok.tolist() and np.allclose(o_st.position, st.position.numpy()) and np.allclose(o_dE, dE2.numpy())
    # streaming average
    W, avg = torch.zeros(2), torch.zeros(2, 2, 3)
    val = torch.arange(12, dtype=torch.float32).reshape(2, 2, 3)
    W1, a1 = streaming_average_update(val, (W, avg), torch.tensor([0.5, 0.0]), torch.tensor([0.0, 1.0]))
    oW, oa = O.streaming_average_update(val.numpy(), (W.numpy(), avg.numpy()), np.array([0.5, 0.0], np.float32), np.array([0.0, 1.0], np.float32))
    assert np.allclose(W1.numpy(), oW) and np.allclose(a1.numpy(), oa)


def test_effective_sample_size_matches_oracle():
    from mile_amd.diagnostics import effective_sample_size
    rng = np.random.default_rng(3)
    for phi, S, C in ((0.9, 2001, 1), (0.0, 500, 1), (0.97, 1500, 3), (-0.4, 999, 2)):
        x = np.zeros((C, S, 6))
        e = rng.standard_normal((C, S, 6))
        for t in range(1, S):
            x[:, t] = phi * x[:, t - 1] + e[:, t]
        got = effective_sample_size(torch.from_numpy(x)).numpy()
        assert np.allclose(got, O.effective_sample_size(x), rtol=1e-9)


def test_lppd_and_predict_match_oracle():
    from mile_amd import ModelSpec
    from mile_amd.metrics import lppd, pointwise_lppd, predict, running_lppd
    for task, hs in (('regr', (8, 8, 2)), ('classification', (8, 5))):
        ospec = O.ModelSpec(4, hs, activation='tanh', task=task)
        spec = ModelSpec(4, hs, activation='tanh', task=task)
        pr = O.synthetic_problem(ospec, 21, 6, seed=5)
        flat = torch.from_numpy(pr['theta0']).double().reshape(2, 3, -1)          # [C, S, d]
        out = predict(spec, flat, torch.from_numpy(pr['X']).double())
        ref = O.mlp_forward(ospec, pr['theta0'].astype(np.float64), pr['X']).reshape(2, 3, 21, -1)
        assert np.allclose(out.numpy(), ref, atol=1e-10)
        pw = pointwise_lppd(torch.from_numpy(ref), torch.from_numpy(pr['y']), task)
        opw = O.pointwise_lppd(ospec, ref, pr['y'])
        assert np.allclose(pw.numpy(), opw, rtol=1e-10, atol=1e-12)
        assert lppd(pw).item() == pytest.approx(O.lppd(opw), rel=1e-12)
        assert running_lppd(pw)[-1].item() == pytest.approx(
            np.log(np.exp(opw).mean(axis=1)).mean(axis=-1).mean(), rel=1e-10)


def test_kernel_factory_rejects_arbitrary_callables():
    from mile_amd.probabilistic import ProbabilisticModel, resolve_target
    from mile_amd import ModelSpec
    with pytest.raises(TypeError, match='ProbabilisticModel'):
        resolve_target(lambda p: 0.0)
    pm = ProbabilisticModel(ModelSpec(5, (8, 2)), task='regr')
    x, y = torch.zeros(4, 5), torch.zeros(4)
    m, xx, yy = resolve_target(pm.bind(x, y))
    assert m is pm and xx is x and yy is y
    m, _, _ = resolve_target(partial(pm.log_unnormalized_posterior, x=x, y=y))
    assert m is pm and pm.spec.prior == 'StandardNormal' and pm.n_params == 66
    with pytest.raises(NotImplementedError, match='Mini-Batch'):
        ProbabilisticModel(ModelSpec(5, (8, 2)), n_batches=2)


# ---------------------------------------------------------------- world_size 2 (gloo) ----
def _dist_worker(rank, ws, port, tmp):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(ws), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist
    from mile_amd import distributed as md
    from mile_amd.metrics import lppd
    dist.init_process_group('gloo', rank=rank, world_size=ws)
    ids = md.shard_chains(np.arange(6), ws, rank)
    assert ids.tolist() == ([0, 1, 2] if rank == 0 else [3, 4, 5])
    g = torch.Generator().manual_seed(0)
    full = torch.randn(4, 6, 7, generator=g)                       # [K, E, d] the whole ensemble
    mine = full[:, ids[0]:ids[-1] + 1].contiguous()
    out, work = md.gather_samples(mine, async_op=True)
    work.wait()
    assert torch.equal(out.contiguous(), full)                     # rank-major == chain order
    pw = torch.randn(6, 5, 9, generator=g)                         # [C, S, N]
    val = md.lppd_distributed(pw[ids[0]:ids[-1] + 1], total_chains=6)
    assert abs(val.item() - lppd(pw).item()) < 1e-6
    torch.save(torch.tensor(1), Path(tmp) / f'ok{rank}')
    dist.barrier()
    dist.destroy_process_group()


def test_sharding_and_sample_collection_world_size_2(tmp_path):
    import torch.multiprocessing as mp
    port = 29600 + os.getpid() % 300
    mp.spawn(_dist_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / 'ok0').exists() and (tmp_path / 'ok1').exists()


def _trainer_worker(rank, ws, port, tmp):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(ws), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist
    from mile_amd import distributed as md
    from mile_amd.config import Config
    from mile_amd.trainer import BDETrainer
    md.init_process_group('gloo')            # host-side control flow: gloo even where a GPU is visible (the trainer reuses the group)
    cfg = Config.from_file(ROOT / 'experiments' / 'mclmc_airfoil_b1.yaml').replace(saving_dir=str(tmp), logging=False)
    names = []
    for _ in range(2):                       # the second construction finds the directory and renames the experiment
        t = BDETrainer(cfg)
        names.append(t.config.experiment_name)
        dist.barrier()
    assert names[0] == 'mclmc_airfoil_3x64' and names[1].startswith('mclmc_airfoil_3x64_'), names
    both = md.gather_objects(names)
    assert both[0] == both[1], both          # every rank derives its paths from rank 0's resolved name
    assert (Path(tmp) / names[1] / 'config.yaml').exists()
    # the per-group files: every rank contributes its chains' values, rank 0 writes them in chain order
    parts = md.gather_objects((np.full(2, rank, dtype=np.float32), np.full(2, 10 + rank, dtype=np.float32)))
    assert [float(v) for p in parts for v in p[0]] == [0.0, 0.0, 1.0, 1.0]
    torch.save(torch.tensor(1), Path(tmp) / f'ok{rank}')
    dist.barrier()
    dist.destroy_process_group()


def test_trainer_ranks_share_the_resolved_experiment_dir_world_size_2(tmp_path):
    """rank 0's setup_dir may rename the experiment; ranks > 0 must not keep the old name."""
    import torch.multiprocessing as mp
    port = 29950 + os.getpid() % 40
    mp.spawn(_trainer_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / 'ok0').exists() and (tmp_path / 'ok1').exists()


def _empty_rank_worker(rank, ws, port, tmp):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(ws), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    import dataclasses
    import torch.distributed as dist
    from mile_amd import distributed as md
    from mile_amd import trainer as T
    from mile_amd.config import Config
    md.init_process_group('gloo')            # host-side control flow: gloo even where a GPU is visible (the trainer reuses the group)
    cfg = Config.from_file(ROOT / 'experiments' / 'mclmc_airfoil_b1.yaml').replace(saving_dir=str(tmp), logging=False)
    smp = dataclasses.replace(cfg.training.sampler, n_chains=1)
    cfg = cfg.replace(training=dataclasses.replace(cfg.training, sampler=smp,
                                                   warmstart=dataclasses.replace(cfg.training.warmstart, include=False)))
    seen = []

    def fake_inference_loop(unnorm_log_posterior, config, rng_key, init_params, step_ids, saving_path, saving_path_warmup=None):
        seen.append(list(step_ids))
        parts = md.gather_objects((np.full(len(step_ids), 0.5, np.float32), np.full(len(step_ids), 7.0, np.float32)))
        assert sum(len(p[0]) for p in parts) == 1              # the group's one chain, from whichever rank owns it
    T.inference_loop = fake_inference_loop
    t = T.BDETrainer(cfg)
    t.start_sampling()                                          # used to raise for 1 chain on 2 ranks
    owners = md.gather_objects(seen)
    assert sorted(len(o) for o in owners) == [0, 1] and [c for o in owners for g in o for c in g] == [0]
    # rank 0 failing in setup_dir must fail every rank, not leave them waiting in the broadcast
    if rank == 0:
        Config.setup_dir = lambda self: (_ for _ in ()).throw(OSError('disk full'))
    try:
        T.BDETrainer(cfg)
        raised = False
    except RuntimeError as exc:
        raised = 'disk full' in str(exc)
    assert raised
    torch.save(torch.tensor(1), Path(tmp) / f'ok{rank}')
    dist.barrier()
    dist.destroy_process_group()


def test_trainer_rank_without_chains_and_setup_failure_world_size_2(tmp_path):
    import torch.multiprocessing as mp
    port = 29300 + os.getpid() % 200
    mp.spawn(_empty_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / 'ok0').exists() and (tmp_path / 'ok1').exists()


def _gather_worker(rank, ws, port, tmp):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(ws), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    sys.path.insert(0, str(ROOT))
    import torch.distributed as dist
    from mile_amd import distributed as md
    dist.init_process_group('gloo', rank=rank, world_size=ws)
    ids = md.shard_chains(np.arange(8), ws, rank)
    g = torch.Generator().manual_seed(1)
    for K, async_op in ((1, False), (5, False), (5, True), (3, True)):      # K kept samples in the chunk
        full = torch.randn(K, 8, 11, generator=g)                          # [K, E, d], chain e = column e
        mine = full[:, ids[0]:ids[-1] + 1].contiguous()
        out, work = md.gather_samples(mine, async_op=async_op)
        if work is not None:
            work.wait()
        got = out.contiguous()
        assert got.shape == full.shape and torch.equal(got, full), (K, async_op)   # sample k, chain order == shard_chains order
    torch.save(torch.tensor(1), Path(tmp) / f'ok{rank}')
    dist.barrier()
    dist.destroy_process_group()


def test_gathered_sample_order_for_several_kept_samples_per_chunk_world_size_2(tmp_path):
    import torch.multiprocessing as mp
    port = 29900 + os.getpid() % 40
    mp.spawn(_gather_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / 'ok0').exists() and (tmp_path / 'ok1').exists()


def test_bench_gpus_n_starts_n_ranks_without_a_launcher():
    """`python bench.py --gpus 2` with no RANK in the environment becomes the launcher: two child ranks, the parent
    never touches the GPU, a failing rank makes the parent fail.  (No GPU here: both ranks refuse loudly.)"""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    r = subprocess.run([sys.executable, str(ROOT / 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1'],
                       capture_output=True, text=True, env=env, timeout=300)
    assert 'started 2 ranks' in r.stderr
    if not torch.cuda.is_available():
        assert r.returncode != 0 and 'needs an MI355X' in r.stderr and r.stdout.strip() == ''
    # under a launcher environment the world size must match --gpus
    env2 = dict(env, RANK='0', WORLD_SIZE='1', LOCAL_RANK='0')
    r2 = subprocess.run([sys.executable, str(ROOT / 'bench.py'), '--gpus', '2'], capture_output=True, text=True, env=env2, timeout=300)
    assert r2.returncode != 0 and 'WORLD_SIZE=1' in r2.stderr


def test_bench_workloads_name_every_baseline_config():
    """bench.py's workloads against BASELINE.json's configs and the oracle's shapes: B2 the default, B3 / B4 / B5 bounded secondary
    legs of the --full run; the FLOP models the roofline fields are priced with against hand counts."""
    import importlib.util, json
    spec = importlib.util.spec_from_file_location('bench_mod', ROOT / 'bench.py')
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from oracle import mclmc_oracle as oracle
    from oracle import lenet_oracle
    assert bench.WORKLOAD == 'B2' and [n for n, _, _ in bench.SECONDARY] == ['B3', 'B4', 'B5']
    assert len(json.loads((ROOT / 'BASELINE.json').read_text())['configs']) == 5
    for name in ('B2', 'B3', 'B4'):
        o, N, E = oracle.config_spec(name)
        assert f'd={o.n_params}' in bench.WORKLOADS[name]['text'] and f'N={N}' in bench.WORKLOADS[name]['text']
    assert bench.WORKLOADS['B2']['ensemble'] == 128 and bench.WORKLOADS['B3']['kernel'] == 'mfma_w128_bf16'
    b5 = bench.WORKLOADS['B5']
    ln = lenet_oracle.LeNetSpec(*b5['image'], b5['classes'])
    assert f'd={ln.n_params}' in b5['text'] and b5['kernel'] == 'lenet_bf16' and b5['ensemble'] * 8 == 256
    # fwd 2 N W + bwd 4 N W - 2 N W0 (no input gradient for the first layer)
    assert bench.grad_flops_per_particle(5, (64, 64, 64, 2), 1052) == 1052 * (6 * (5 * 64 + 64 * 64 * 2 + 64 * 2) - 2 * 5 * 64)
    m1, m2, md = 32 * 32 * 75 * 6, 12 * 12 * 150 * 16, 576 * 120 + 120 * 84 + 84 * 10
    assert bench.lenet_grad_flops_per_particle(3, 32, 32, 10, 4000) == 4000 * (6 * (m1 + m2 + md) - 2 * m1)


def test_bench_extras_only_with_full():
    """bench.py's --full (roofline pass, CPU baseline, secondary legs) is off by default and combines with the --no-* options
    that drop parts of it; what each run prints is checked on the GPU in tests/test_gpu_bench.py."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_mod', ROOT / 'bench.py')
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    ap = bench.arg_parser()
    plain = ap.parse_args(['--gpus', '1', '--steps', '20', '--warmup', '5'])
    assert not plain.full and (plain.steps, plain.warmup) == (20, 5)
    full = ap.parse_args(['--full', '--no-secondary'])
    assert full.full and full.no_secondary and not full.no_cpu_baseline and not full.no_kernel_timing


def test_bench_dump_outputs_within_budget_and_fixed_sample(tmp_path):
    """bench.py --dump-outputs: float32 .npy per returned array; under the budget every array is written whole, over it every
    [..., d] array keeps the same seeded column sample (identical from run to run) and the files stay within the budget."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_mod', ROOT / 'bench.py')
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(3)
    E, d = 8, 1000
    arrays = {'position': rng.standard_normal((E, d)), 'logdensity': rng.standard_normal(E),
              'samples': rng.standard_normal((2, E, d)).astype(np.float32)}
    m = bench.dump_outputs(tmp_path / 'whole', arrays, d)
    assert m['param_columns'] is None
    for name, a in arrays.items():
        got = np.load(tmp_path / 'whole' / f'{name}.npy')
        assert got.dtype == np.float32 and np.array_equal(got, a.astype(np.float32))
    budget = 40_000
    for run in ('a', 'b'):
        m = bench.dump_outputs(tmp_path / run, arrays, d, budget=budget)
        assert m['param_columns'] is not None
        assert sum(f.stat().st_size for f in (tmp_path / run).iterdir()) <= budget + 3 * 128   # + .npy headers
    k = np.load(tmp_path / 'a' / 'position.npy').shape[1]
    assert 0 < k < d and np.load(tmp_path / 'a' / 'samples.npy').shape == (2, E, k)
    assert np.array_equal(np.load(tmp_path / 'a' / 'logdensity.npy'), arrays['logdensity'].astype(np.float32))
    cols = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(d, k, replace=False))
    for name in ('position', 'samples'):
        a, b = np.load(tmp_path / 'a' / f'{name}.npy'), np.load(tmp_path / 'b' / f'{name}.npy')
        assert np.array_equal(a, b) and np.array_equal(a, arrays[name][..., cols].astype(np.float32))


def test_airfoil_table_loads_with_reference_split():
    """The shipped data fixture behind experiments/mclmc_airfoil_b1/b2.yaml (data/README.md): 1503 x 6, z-scored
    including the target (tabular.py:146-147), 70 / 10 / 20 split -> N_train = 1052."""
    from mile_amd.config import Config
    from mile_amd.dataset import TabularLoader
    raw = np.genfromtxt(ROOT / 'data' / 'airfoil.data', delimiter=' ')
    assert raw.shape == (1503, 6) and np.isfinite(raw).all()
    assert raw[0].tolist() == [800.0, 0.0, 0.3048, 71.3, 0.00266337, 126.201]
    cfg = Config.from_file(ROOT / 'experiments' / 'mclmc_airfoil_b2.yaml')
    assert cfg.data.path == 'data/airfoil.data' and cfg.data.source == 'local'
    cwd = os.getcwd()
    try:
        os.chdir('/')                                   # relative path resolves against the repository root too
        ld = TabularLoader(cfg.data, rng=cfg.rng)
    finally:
        os.chdir(cwd)
    assert ld.train_x.shape == (1052, 5) and ld.valid_x.shape == (150, 5) and ld.test_x.shape == (301, 5)
    allx = np.concatenate([ld.train_x, ld.valid_x, ld.test_x]); ally = np.concatenate([ld.train_y, ld.valid_y, ld.test_y])
    assert np.abs(allx.mean(0)).max() < 1e-4 and np.abs(allx.std(0) - 1).max() < 1e-4
    assert abs(ally.mean()) < 1e-4 and abs(ally.std() - 1) < 1e-4


def test_unsupported_activations_are_config_errors():
    from mile_amd.config import Config, ConfigError
    d = Config.from_file(ROOT / 'experiments' / 'mclmc_airfoil_b1.yaml').to_dict()
    for act in ('gelu', 'leaky_relu', 'softmax'):
        d['model']['activation'] = act
        with pytest.raises(ConfigError, match='not implemented'):
            Config.from_dict(d)


def test_chain_ess_metric_rank_normalised():
    """src/inference/metrics.py:226-244,386-405: pooled rank normalisation, then one single-chain ESS per chain."""
    from scipy.stats import norm, rankdata
    from mile_amd.metrics import effective_sample_size, rank_normalize_array
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 400, 2, generator=g, dtype=torch.float64)
    x[0, 0, 0] = x[1, 1, 0]                                                  # a tie gets the average rank
    r = rank_normalize_array(x[:, :, 0]).numpy()
    ref = norm.ppf((rankdata(x[:, :, 0].numpy(), axis=None).reshape(3, 400) - 0.375) / (1200 + 0.25))
    assert np.abs(r - ref).max() < 1e-9
    ess = effective_sample_size(x)
    assert ess.shape == (3, 2) and 250 < float(ess.min()) and float(ess.max()) < 650      # white noise: ESS ~ S
    rho = 0.9                                                                # AR(1): ESS ~ S (1 - rho) / (1 + rho)
    z = torch.randn(2, 4000, generator=g, dtype=torch.float64)
    y = torch.zeros_like(z)
    for t in range(1, 4000):
        y[:, t] = rho * y[:, t - 1] + z[:, t]
    e2 = effective_sample_size(y[:, :, None])[:, 0]
    assert torch.all((e2 > 0.5 * 4000 * 0.1 / 1.9) & (e2 < 2.0 * 4000 * 0.1 / 1.9)), e2
    # the oracle's estimator on the same rank-normalised column
    rn = rank_normalize_array(y).numpy()
    eo = np.stack([np.asarray(O.effective_sample_size(rn[c][None, :, None])).reshape(-1)[0] for c in range(2)])
    assert np.abs(e2.numpy() - eo).max() / eo.max() < 1e-6


class _FakeEngine:
    """Records what the tuner asks of the engine (no GPU): eng.tune advances nothing."""

    def __init__(self, d):
        self.device, self.d, self.supports_device_tuner = torch.device('cpu'), d, True
        self.tune_calls = []

    def tune(self, state, tuner, L, n_steps, **kw):
        self.tune_calls.append((torch.as_tensor(L).clone(), n_steps, kw['sqrt_diag_cov']))
        tuner['stream_average'][:, 0] = 1.0
        tuner['stream_average'][:, 1] = 5.0          # variances = 4 -> sqrt_diag_cov = 2


def test_readjustment_runs_with_the_phase1_L_and_returns_sqrt_dim():
    """src/training/warmup.py:389-403: under diagonal_preconditioning only params.sqrt_diag_cov is
    replaced before the re-adjustment run_steps, so its kernel steps keep L = max(sqrt(d), 15); sqrt(d) is returned."""
    from mile_amd.engine import IntegratorState
    from mile_amd.warmup import mclmc_find_L_and_step_size
    E, d = 2, 138                                    # d < 225: sqrt(d) = 11.7 < 15
    eng = _FakeEngine(d)
    st = IntegratorState(torch.zeros(E, d), torch.zeros(E, d), torch.zeros(E), torch.zeros(E, d))
    _, params = mclmc_find_L_and_step_size(eng, st, 0, tune1_steps=8, tune2_steps=6, tune3_steps=0, step_size_init=0.01,
                                           desired_energy_var_start=0.5, desired_energy_var_end=0.1, trust_in_estimate=1.5,
                                           num_effective_samples=100, diagonal_preconditioning=True)
    (L1, n1, s1), (L2, n2, s2) = eng.tune_calls
    assert n1 == 14 and s1 is None and torch.all(L1 == 15.0)
    assert n2 == 2 and torch.all(L2 == 15.0) and torch.allclose(s2, torch.full((E, d), 2.0))   # phase-1 L, new preconditioner
    assert torch.allclose(params.L, torch.full((E,), math.sqrt(d))) and torch.allclose(params.sqrt_diag_cov, s2)


def test_padded_lds_image_maps_are_conflict_free_and_transpose_correctly():
    """The index algebra of the padded bf16 LDS images (mile_amd/csrc/mile_bf16_frag.h, pim_*), restated and run against the
    LDS model of the MI355X guide: ds_read_b128 is served in four 16-lane groups, ds_read_b64_tr_b16 in two 32-lane groups,
    64 banks of 4 bytes, one cycle per group when no two lanes of a group touch different addresses of one bank.  Checks
    (a) both read kinds are conflict-free at the 272-byte pitch (and the transposed read at the 144-byte pitch of the
    64-column images of k_grad_w64), (b) the transposed read returns element j of lane (r, h) = image[row0 + 8h + j][col0 + r]
    under the instruction's own lane semantics (lane 4q + p of a 16-lane group supplies the address of row q, columns
    4p..4p+3; lane i receives column i of the four rows), (c) the constants in the header are the ones modelled here."""
    hdr = (Path(__file__).resolve().parents[1] / 'mile_amd' / 'csrc' / 'mile_bf16_frag.h').read_text()
    assert '#define PIM_STRIDE 272' in hdr
    assert 'return (i & ~15) | ((i & 3) << 2) | (((i >> 3) & 1) << 1) | ((i >> 2) & 1);' in hdr
    assert 'return STRIDE * (4 * q + 2 * h) + 32 * g1 + 16 * (p >> 1) + 8 * (p & 1);' in hdr

    def pim_row(i):
        return (i & ~15) | ((i & 3) << 2) | (((i >> 3) & 1) << 1) | ((i >> 2) & 1)

    def tr_base(lane, stride):
        h, g1, q, p = lane >> 5, (lane >> 4) & 1, (lane & 15) >> 2, lane & 3
        return stride * (4 * q + 2 * h) + 32 * g1 + 16 * (p >> 1) + 8 * (p & 1)

    assert sorted(pim_row(i) for i in range(32)) == list(range(32))          # a permutation inside each 16-row group
    assert all(pim_row(i) >> 4 == i >> 4 for i in range(64))

    def banks_ok(addrs_by_lane, groups, nbytes):
        for g in groups:
            seen = {}
            for lane in g:
                for dw in range(nbytes // 4):
                    a = addrs_by_lane[lane] + 4 * dw
                    b = (a // 4) % 64
                    if seen.setdefault(b, a) != a:
                        return False
        return True

    b128_groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    b128_groups += [[l + 32 for l in g] for g in b128_groups]
    tr_groups = [list(range(32)), list(range(32, 64))]
    for s in range(8):            # row read of k-step s: lane (r, h) takes chunk 2 s + h of row r
        addrs = [272 * pim_row(l & 31) + 16 * (2 * s + (l >> 5)) for l in range(64)]
        assert banks_ok(addrs, b128_groups, 16)
        swz = [256 * (l & 31) + 16 * (2 * s + (l >> 5)) for l in range(64)]      # the unpadded, unpermuted image conflicts
        assert not banks_ok(swz, b128_groups, 16)
    for stride, ncols in ((272, 128), (144, 64)):
        img = np.arange(32 * ncols, dtype=np.int64).reshape(32, ncols)           # logical image: value = 128 row + col
        phys = {}                                                                 # byte address -> element
        for row in range(32):
            for col in range(ncols):
                phys[stride * pim_row(row) + 2 * col] = img[row, col]
        for row0 in (0, 16):
            for col0 in range(0, ncols, 32):
                for t in (0, 1):                                                  # the fragment's two reads
                    addrs = [tr_base(l, stride) + stride * row0 + 2 * col0 + stride * t for l in range(64)]
                    assert banks_ok(addrs, tr_groups, 8)
                    for lane in range(64):
                        grp, i = lane & ~15, lane & 15
                        for q in range(4):                                        # lane receives column i of the group's 4 rows
                            src = grp + 4 * q + (i >> 2)                          # the lane that supplied row q, columns 4(i>>2)..
                            got = phys[addrs[src] + 2 * (i & 3)]
                            r, h, j = lane & 31, lane >> 5, 4 * t + q
                            assert got == img[row0 + 8 * h + j, col0 + r], (stride, row0, col0, t, lane, q)
