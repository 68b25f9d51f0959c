"""AttentionClassifier at emb_size 192 (WideAttentionSpec, k_grad_attn_wide) without a GPU: reference sizes, the factory that keeps
every earlier shape on k_grad_attn, the two pretraining experiments, spec / library agreement over the envelope, kernel choice,
and the condition of the per-leaf GPU check (every leaf's gradient is the likelihood's) on the fp64 restatement alone."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from tests import attn_ref as A
from tests import leaf_cases as LC
from tests import leafcheck as L

ROOT = Path(__file__).resolve().parents[1]

STOCK = (10000, 70, 192, 8, 64, 2, (32,), True)
LARGER = (10000, 70, 192, 10, 100, 2, (128, 32), True)
# the problems of tests/test_gpu_attn_wide.py::test_gradient_per_leaf: V, T, C, H, D, K, proj, bias, N, E
LEAF_CASES = [
    (300, 24, 192, 8, 64, 2, (32,), True, 24, 2),
    (300, 24, 192, 10, 100, 2, (128, 32), True, 20, 2),
    (97, 33, 130, 5, 80, 3, (), False, 17, 2),
    STOCK + (24, 1),
    LARGER + (20, 1),
]


def wide_spec(V, T, Cc, H, D, K=2, proj=(32,), bias=True, prior='Normal', scale=0.2):
    from mile_amd.spec import WideAttentionSpec
    return WideAttentionSpec(V, T, Cc, H, D, n_classes=K, projection_dim=proj, use_bias=bias, prior=prior, prior_scale=scale)


def leaf_problem(V, T, Cc, H, D, K, proj, bias, N, E):
    spec = wide_spec(V, T, Cc, H, D, K, proj, bias, scale=LC.ATTN_PRIOR_SCALE)
    return LC.AttnProblem('attn', spec, A.sharp_problem(spec, N, E, LC.SEED))


def test_reference_sizes_leaves_and_factory():
    from mile_amd import WideAttentionSpec as exported
    from mile_amd.spec import NATIVE_SPECS, AttentionSpec, WideAttentionSpec, attention_spec
    assert exported is WideAttentionSpec and WideAttentionSpec in NATIVE_SPECS
    stock = WideAttentionSpec(10000, 70, 192, 8, 64, use_bias=True)
    larger = WideAttentionSpec(10000, 70, 192, 10, 100, projection_dim=(128, 32), use_bias=True)
    assert stock.n_params == 1_989_218 and larger.n_params == 2_039_630
    small = AttentionSpec(1000, 70, 48, 8, 64, use_bias=True)
    forced = WideAttentionSpec(1000, 70, 48, 8, 64, use_bias=True)
    assert forced.leaves() == small.leaves() and forced.n_params == small.n_params
    assert [n for n, _, _ in stock.leaves()] == [n for n, _, _ in small.leaves()]
    assert stock.flops_per_sequence == 3 * 8_148_096        # 24.44 MFLOP: 0.855 TFLOP per gradient of N = 35 000 rows
    assert stock.lds_bytes <= 160 * 1024 and larger.lds_bytes <= 160 * 1024
    kw = dict(n_heads=8, qkv_dim=64, use_bias=True)
    assert type(attention_spec(vocab_size=1000, context_len=70, emb_size=48, **kw)) is AttentionSpec
    assert type(attention_spec(vocab_size=10000, context_len=70, emb_size=192, **kw)) is WideAttentionSpec
    assert type(attention_spec(vocab_size=10000, context_len=70, emb_size=192, n_heads=10, qkv_dim=100, projection_dim=(128, 32),
                               use_bias=True)) is WideAttentionSpec
    with pytest.raises(NotImplementedError):
        AttentionSpec(1000, 70, 192, 8, 64)
    with pytest.raises(NotImplementedError, match='emb_size'):
        attention_spec(vocab_size=100, context_len=16, emb_size=193, n_heads=2, qkv_dim=16)
    # slab sizing at the stock shape: one chain takes a workgroup per CU, eight chains 32 ranges each -- 2.04 GB either way;
    # a 256-row minibatch is cut into 32 ranges
    assert stock.row_splits(1, 35000) == 256 and stock.row_splits(8, 35000) == 32 and stock.row_splits(1, 256) == 32
    assert stock.slab_bytes(1, 35000) == stock.slab_bytes(8, 35000) == 256 * 1_989_220 * 4


# the reference's two pretraining files, field for field: the larger one also trains longer (adamw 0.001 without weight decay,
# 20 epochs), samples longer (50 000 / 10 000) and has the wider prior
@pytest.mark.parametrize('name,heads,qkv,proj,opt,epochs,warmup,n_samples,scale',
                         [('mclmc_seqmod_pretraining_synthetic.yaml', 8, 64, [32], {'learning_rate': 0.01, 'weight_decay': 0.001},
                           2, 5000, 1000, 0.2),
                          ('mclmc_seqmod_pretraining_larger_synthetic.yaml', 10, 100, [128, 32], {'learning_rate': 0.001},
                           20, 50000, 10000, 0.4)])
def test_pretraining_experiments_parse(name, heads, qkv, proj, opt, epochs, warmup, n_samples, scale):
    import yaml
    from mile_amd.config import AttentionClassifierConfig, Config
    from mile_amd.spec import WideAttentionSpec
    from mile_amd.trainer import BDETrainer
    path = ROOT / 'experiments' / name
    cfg = Config.from_file(path)
    m = cfg.model
    assert type(m) is AttentionClassifierConfig
    assert (m.vocab_size, m.context_len, m.emb_size, m.n_heads, m.qkv_dim, m.bias, m.n_classes) == (10000, 70, 192, heads, qkv, True, 2)
    assert m.projection_dim == proj
    assert cfg.data.data_type == 'text' and cfg.data.path == '50000x70x10000'
    ws, sm = cfg.training.warmstart, cfg.training.sampler
    assert (ws.include, ws.optimizer_config.name, ws.max_epochs, ws.batch_size) == (True, 'adamw', epochs, 256)
    assert ws.optimizer_config.parameters == opt
    assert (sm.name, sm.warmup_steps, sm.n_samples, sm.n_thinning, sm.n_chains) == ('mclmc', warmup, n_samples, 100, 1)
    assert sm.prior_config.name == 'Normal' and sm.prior_config.parameters == {'loc': 0.0, 'scale': scale}
    assert cfg.n_chains == 1
    raw = yaml.safe_load(path.read_text())
    raw['data']['path'] = '64x24x200'
    raw['data']['datapoint_limit'] = 64
    raw['model'].update(vocab_size=200, context_len=24)
    small = Config.from_dict(raw) if hasattr(Config, 'from_dict') else None
    if small is None:
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            (Path(td) / 'c.yaml').write_text(yaml.safe_dump(raw))
            small = Config.from_file(Path(td) / 'c.yaml')
    t = BDETrainer.__new__(BDETrainer)
    t.build_model(small)
    assert type(t.spec_model) is WideAttentionSpec and t.spec_model.emb_size == 192 and t.spec_model.qkv_dim == qkv
    assert t.prob_model.spec.n_params == t.spec_model.n_params


def _cspec(V, T, Cc, H, D, proj, K, bias=1, model=5):
    from mile_amd import _lib
    cs = _lib.ModelSpecC()
    cs.in_features = T
    widths = list(proj) + [K]
    cs.n_layers = len(widths)
    for i, w in enumerate(widths):
        cs.widths[i] = w
    cs.task, cs.prior, cs.prior_scale, cs.use_bias = 1, 0, 1.0, bias
    cs.model, cs.vocab_size, cs.ctx_len, cs.emb_size, cs.n_heads, cs.qkv_dim = model, V, T, Cc, H, D
    return cs


def _create(cs):
    from mile_amd import _lib
    lib = _lib.load_library()
    h = C.c_void_p()
    rc = lib.mile_create(C.byref(cs), 0, C.byref(h))
    return lib, h, rc


ENVELOPE = [(T, Cc, H, D, proj) for T in (1, 16, 37, 70, 96, 112, 128) for Cc in (8, 61, 192) for (H, D) in
            ((1, 8), (8, 64), (10, 100), (1, 100), (4, 128), (3, 57)) for proj in ((), (32,), (128, 32))]


def test_spec_and_library_agree_over_the_envelope():
    from mile_amd.spec import WideAttentionSpec
    ok = refused = 0
    for bias in (True, False):
        for T, Cc, H, D, proj in ENVELOPE + [(70, 193, 8, 64, ()), (129, 16, 2, 16, ()), (16, 16, 1, 129, ()),
                                             (16, 16, 2, 16, (129,)), (16, 16, 2, 16, (8, 8, 8))]:
            try:
                spec = WideAttentionSpec(100, T, Cc, H, D, projection_dim=proj, use_bias=bias)
                want, why = True, ''
            except NotImplementedError as exc:
                want, why = False, str(exc)
            lib, h, rc = _create(_cspec(100, T, Cc, H, D, proj, 2, int(bias)))
            assert (rc == 0) == want, (T, Cc, H, D, proj, rc, lib.mile_last_error())
            if rc == 0:
                assert lib.mile_param_count(h) == spec.n_params
                bo, ko = C.c_int64(), C.c_int64()
                leaves = {n: o for n, o, _ in spec.leaves()}
                names = (['MDPA.key', 'MDPA.out', 'MDPA.query', 'MDPA.value', 'TokenEmbedding_0.Embedding', 'TokenEmbedding_0.PositionEmbedding',
                          'classifier'] + [f'projection_{i}' for i in range(len(proj))])
                for layer, name in enumerate(names):
                    assert lib.mile_param_offsets(h, layer, C.byref(bo), C.byref(ko)) == 0
                    table = 'Embedding' in name
                    assert ko.value == leaves[f'{name}.embedding' if table else f'{name}.kernel']
                    assert bo.value == (leaves[f'{name}.bias'] if bias and not table else -1)
                assert lib.mile_destroy(h) == 0
                ok += 1
            else:
                refused += 1
                if T <= 128 and Cc <= 192 and D <= 128 and len(proj) <= 2 and all(p <= 128 for p in proj):
                    assert 'LDS' in why and b'LDS' in lib.mile_last_error(), (T, Cc, H, D, proj, why)
    assert ok > 200 and refused > 10
    with pytest.raises(NotImplementedError, match='LDS'):
        WideAttentionSpec(10000, 112, 192, 8, 64)
    # token ids travel as fp32: both sides stop at the same vocabulary
    for V, want in (((1 << 24) - 1, True), (1 << 24, False)):
        try:
            n = WideAttentionSpec(V, 16, 8, 2, 16, projection_dim=()).n_params
        except NotImplementedError as exc:
            n = None
            assert 'vocab_size' in str(exc)
        lib, h, rc = _create(_cspec(V, 16, 8, 2, 16, (), 2, 0))
        assert (rc == 0) == want == (n is not None), (V, rc, lib.mile_last_error())
        if rc == 0:
            assert lib.mile_param_count(h) == n
            lib.mile_destroy(h)
        else:
            assert b'vocab_size' in lib.mile_last_error()


def test_kernel_choice_without_a_gpu():
    """AUTO resolves model 5 to ATTN_WIDE_F32 (14), the only kernel it accepts; every other model refuses 14."""
    from mile_amd import _lib
    assert _lib.ABI_VERSION == 10 and _lib.MODEL_IDS['attn_wide'] == 5
    lib, h, rc = _create(_cspec(50, 16, 32, 2, 16, (8,), 2))
    assert rc == 0, lib.mile_last_error()
    try:
        assert lib.mile_get_grad_kernel(h) == _lib.GRAD_KERNEL_IDS['attn_wide_f32'] == 14
        for k in range(1, 15):
            rc = lib.mile_set_grad_kernel(h, k)
            assert (rc == 0) == (k == 14), (k, lib.mile_last_error())
            assert lib.mile_set_grad_kernel(h, 0) == 0
        assert lib.mile_set_grad_kernel(h, 15) == -1
        buf = (C.c_float * 4)()
        assert lib.mile_set_embedding(h, buf, buf, None) == -1          # its tables are parameters
    finally:
        lib.mile_destroy(h)
    others = []
    for model in (3, 4):
        others.append(_cspec(50, 16, 32, 2, 16, (8,), 2, model=model))
    fcn = _lib.ModelSpecC()
    fcn.in_features, fcn.n_layers, fcn.task, fcn.prior_scale, fcn.use_bias, fcn.model = 4, 2, 0, 1.0, 1, 0
    fcn.widths[0], fcn.widths[1] = 8, 2
    others.append(fcn)
    for shape, model in (((1, 12, 14), 1), ((1, 8, 8), 2)):
        img = _lib.ModelSpecC()
        img.in_features, img.n_layers, img.task, img.prior_scale, img.use_bias, img.model = int(np.prod(shape)), 1, 1, 1.0, 1, model
        img.widths[0] = 3
        img.img_c, img.img_h, img.img_w = shape
        others.append(img)
    seen = set()
    for cs in others:
        lib, h, rc = _create(cs)
        if rc != 0 and cs.model == 1:                                   # LeNet needs rocBLAS to load: not this test's matter
            continue
        assert rc == 0, (cs.model, lib.mile_last_error())
        try:
            assert lib.mile_set_grad_kernel(h, 14) == -1
            assert b'ATTN_WIDE_F32 is the kernel of MILE_MODEL_ATTN_WIDE' in lib.mile_last_error()
            seen.add(cs.model)
        finally:
            lib.mile_destroy(h)
    assert {0, 2, 3, 4} <= seen


def test_config_takes_the_kernel_name():
    from mile_amd.config import ConfigError, SamplerConfig
    assert SamplerConfig(grad_kernel='attn_wide_f32').grad_kernel == 'attn_wide_f32'
    with pytest.raises(ConfigError):
        SamplerConfig(grad_kernel='attn_wider_f32')


@pytest.mark.parametrize('case', LEAF_CASES[:3] + [pytest.param(c, id=f'full-{i}') for i, c in enumerate(LEAF_CASES[3:])])
def test_every_leaf_is_the_likelihoods(case):
    """The condition of the per-leaf GPU check, on the restatement alone: under prior_scale 1000 every leaf of every chain has
    max |likelihood gradient| >= 0.5 max |gradient| (leaf_cases.MIN_SHARE), and the float32 restatement's own error is small."""
    P = leaf_problem(*case)
    _, g = P.ref()
    share = L.likelihood_share(P.lik(), g, P.leaves)
    keep = np.array([n != LC.KEY_BIAS for n, _, _ in P.leaves])        # zero analytically: compared on the query bias's scale
    assert share[:, keep].min() >= LC.MIN_SHARE, (case, share.min(axis=0))
    _, g32 = P.ref(np.float32)
    assert L.leaf_errors(g32, g, P.leaves, P.scale_of).max() < 1e-4
