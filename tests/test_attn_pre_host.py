"""PretrainedAttentionClassifier without a GPU: the fp64 restatement against torch autograd, the extra gelu, parameter layout,
the table path rule and validation, config parsing, spec / library agreement and tools/make_embeddings.py."""
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests import attn_pre_ref as R
from tests import attn_ref as A

ROOT = Path(__file__).resolve().parents[1]


def _spec(V=40, T=12, C=16, H=4, D=16, K=3, proj=(8,), bias=True, emb_path=None):
    from mile_amd.spec import PretrainedAttentionSpec
    return PretrainedAttentionSpec(V, T, C, H, D, n_classes=K, projection_dim=proj, use_bias=bias, emb_path=emb_path)


@pytest.mark.parametrize('proj,bias', [((8,), True), ((), False), ((12, 6), True)])
def test_restatement_matches_torch_autograd(proj, bias):
    torch = pytest.importorskip('torch')
    spec = _spec(proj=proj, bias=bias)
    prob = R.synthetic_problem(spec, 9, 1, seed=2)
    th = prob['theta0'][0].astype(np.float64)
    ll, g = R.loglik_and_grad(spec, th, prob['emb'], prob['pos'], prob['x'], prob['y'])
    T, Cc, H, D = spec.context_len, spec.emb_size, spec.n_heads, spec.qkv_dim
    hd = D // H
    t = torch.tensor(th, requires_grad=True)
    P = {n: t[o:o + int(np.prod(s))].reshape(s) for n, o, s in spec.leaves()}
    x = torch.tensor(prob['x'])
    e = torch.tensor(prob['emb'], dtype=torch.float64)[x] + torch.tensor(prob['pos'], dtype=torch.float64)[None, :T]
    dense = lambda name: e @ P[f'MDPA.{name}.kernel'].reshape(Cc, D) + (P[f'MDPA.{name}.bias'].reshape(D) if bias else 0)  # noqa: E731
    heads = lambda a: a.reshape(-1, T, H, hd).transpose(1, 2)                                                          # noqa: E731
    q, k, v = heads(dense('query')) / np.sqrt(hd), heads(dense('key')), heads(dense('value'))
    m = x != 0
    mask = (m[:, :, None] & m[:, None, :])[:, None]
    s = torch.where(mask, q @ k.transpose(-1, -2), torch.tensor(float(np.finfo(np.float32).min), dtype=torch.float64))
    o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(-1, T, D)
    z = (o @ P['MDPA.out.kernel'].reshape(D, Cc) + (P['MDPA.out.bias'] if bias else 0)).mean(1)
    gelu = lambda a: torch.nn.functional.gelu(a, approximate='tanh')                                                   # noqa: E731
    for i in range(len(proj)):
        z = gelu(z @ P[f'projection_{i}.kernel'] + (P[f'projection_{i}.bias'] if bias else 0))
    lg = gelu(z) @ P['classifier.kernel'] + (P['classifier.bias'] if bias else 0)
    llt = torch.log_softmax(lg, -1)[torch.arange(len(lg)), torch.tensor(prob['y'], dtype=torch.long)].sum()
    llt.backward()
    assert abs(ll - llt.item()) < 1e-10 * max(1.0, abs(ll))
    assert np.abs(g - t.grad.numpy()).max() < 1e-10 * np.abs(g).max()


def test_extra_gelu_is_the_difference():
    """Same weights, same e: the AttentionClassifier restatement's logits are classifier(z); this model's are
    classifier(gelu(z)) -- different, and equal once the gelu is applied by hand."""
    from mile_amd.spec import AttentionSpec
    spec = _spec()
    full = AttentionSpec(spec.vocab_size, spec.context_len, spec.emb_size, spec.n_heads, spec.qkv_dim, n_classes=spec.n_classes,
                         projection_dim=spec.projection_dim, use_bias=True)
    prob = R.synthetic_problem(spec, 7, 1, seed=5)
    P = R.params(spec, prob['theta0'][0], prob['emb'], prob['pos'])
    f_pre = R.forward(spec, P, prob['x'])
    f_att = A._forward(full, P, prob['x'])
    assert np.abs(f_pre['logits'] - f_att['logits']).max() > 1e-3
    z = f_att['zs'][-1]
    by_hand = A._gelu(z)[0] @ P['classifier.kernel'] + P['classifier.bias']
    np.testing.assert_allclose(f_pre['logits'], by_hand, rtol=1e-12, atol=1e-12)


def test_leaves_and_reference_sizes():
    from mile_amd.spec import PretrainedAttentionSpec
    stock = PretrainedAttentionSpec(10000, 70, 192, 8, 64, projection_dim=(32,), use_bias=True)
    larger = PretrainedAttentionSpec(10000, 70, 192, 10, 100, projection_dim=(128, 32), use_bias=True)
    assert stock.n_params == 55778 and larger.n_params == 106190
    names = [n for n, _, _ in stock.leaves()]
    assert names == ['MDPA.key.bias', 'MDPA.key.kernel', 'MDPA.out.bias', 'MDPA.out.kernel', 'MDPA.query.bias',
                     'MDPA.query.kernel', 'MDPA.value.bias', 'MDPA.value.kernel', 'classifier.bias', 'classifier.kernel',
                     'projection_0.bias', 'projection_0.kernel']
    shapes = {n: s for n, _, s in larger.leaves()}
    assert shapes['MDPA.key.kernel'] == (192, 10, 10) and shapes['MDPA.out.kernel'] == (10, 10, 192)
    assert shapes['projection_0.kernel'] == (192, 128) and shapes['projection_1.kernel'] == (128, 32)
    assert shapes['classifier.kernel'] == (32, 2)
    nobias = PretrainedAttentionSpec(10000, 70, 192, 8, 64)
    assert all(n.endswith('kernel') for n, _, _ in nobias.leaves())
    # the FLOP model: 3 x forward minus the input-gradient product (19.3 / 30.2 MFLOP per sequence and chain)
    assert stock.flops_per_sequence == 19283328 and larger.flops_per_sequence == 30244416


def test_table_path_rule(tmp_path):
    """str.replace('emb', 'pos_emb') over the whole path, directories included."""
    from mile_amd.spec import pretrained_table_paths
    assert pretrained_table_paths('results/pretrained_seq/emb.npy') == ('results/pretrained_seq/emb.npy',
                                                                        'results/pretrained_seq/pos_emb.npy')
    assert pretrained_table_paths('results/pretrained_seq/emb_large.npy')[1] == 'results/pretrained_seq/pos_emb_large.npy'
    assert pretrained_table_paths('embeddings/emb.npy')[1] == 'pos_embeddings/pos_emb.npy'
    assert pretrained_table_paths(Path('a/emb.npy'))[1] == 'a/pos_emb.npy'
    # a directory whose name holds 'emb': the position table is looked up in the rewritten directory, as the reference does
    spec = _spec()
    emb, pos = R.tables(spec)
    d = tmp_path / 'embdir'
    d.mkdir()
    np.save(d / 'emb.npy', emb)
    np.save(d / 'pos_emb.npy', pos)
    assert 'emb' not in str(tmp_path)                  # (pytest names the directory after the test)
    with pytest.raises(FileNotFoundError, match='pos_embdir'):
        _spec(emb_path=str(d / 'emb.npy')).load_tables()
    (tmp_path / 'pos_embdir').mkdir()
    np.save(tmp_path / 'pos_embdir' / 'pos_emb.npy', pos)
    e2, p2 = _spec(emb_path=str(d / 'emb.npy')).load_tables()
    assert np.array_equal(e2, emb) and np.array_equal(p2, pos)


def test_tables_validated_and_cast(tmp_path):
    spec = _spec()
    emb, pos = R.tables(spec, extra_pos_rows=5)
    np.save(tmp_path / 'emb.npy', emb.astype(np.float64))
    np.save(tmp_path / 'pos_emb.npy', pos.astype(np.float16))
    e, p = _spec(emb_path=str(tmp_path / 'emb.npy')).load_tables()
    assert e.dtype == np.float32 and p.dtype == np.float32 and p.shape == (spec.context_len, spec.emb_size)
    assert e.flags['C_CONTIGUOUS'] and p.flags['C_CONTIGUOUS']
    np.testing.assert_array_equal(p, pos[:spec.context_len].astype(np.float16).astype(np.float32))
    with pytest.raises(ValueError, match='embedding table'):
        spec.check_tables(emb[:-1], pos)
    with pytest.raises(ValueError, match='embedding table'):
        spec.check_tables(emb[:, :-1], pos)
    with pytest.raises(ValueError, match='position table'):
        spec.check_tables(emb, pos[:spec.context_len - 1])
    with pytest.raises(ValueError, match='position table'):
        spec.check_tables(emb, pos[:, :-1])
    bad = emb.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match='finite'):
        spec.check_tables(bad, pos)
    with pytest.raises(ValueError, match='emb_path'):
        spec.load_tables()
    with pytest.raises(FileNotFoundError, match='make_embeddings'):
        _spec(emb_path=str(tmp_path / 'missing' / 'x.npy')).load_tables()


@pytest.mark.parametrize('name,heads,qkv,proj,scale,emb',
                         [('mclmc_seqmod_pretrained_synthetic.yaml', 8, 64, [32], 0.2, 'emb.npy'),
                          ('mclmc_seqmod_pretrained_larger_synthetic.yaml', 10, 100, [128, 32], 0.4, 'emb_large.npy')])
def test_config_parses_the_new_experiments(name, heads, qkv, proj, scale, emb):
    from mile_amd.config import Config, PretrainedAttentionClassifierConfig
    cfg = Config.from_file(ROOT / 'experiments' / name)
    m = cfg.model
    assert isinstance(m, PretrainedAttentionClassifierConfig)
    assert (m.vocab_size, m.context_len, m.emb_size, m.n_heads, m.qkv_dim, m.bias, m.n_classes) == (10000, 70, 192, heads, qkv,
                                                                                                     True, 2)
    assert m.projection_dim == proj and m.emb_path == f'results/pretrained_seq/{emb}'
    assert cfg.data.data_type == 'text' and cfg.data.path == '50000x70x10000'
    assert cfg.training.sampler.prior_config.parameters['scale'] == scale
    assert cfg.n_chains == 8 and cfg.rng == 123


def test_config_needs_emb_path():
    from mile_amd.config import ConfigError, PretrainedAttentionClassifierConfig
    with pytest.raises(ConfigError, match='emb_path'):
        PretrainedAttentionClassifierConfig(vocab_size=100, context_len=8, emb_size=16, n_heads=2, qkv_dim=16)
    c = PretrainedAttentionClassifierConfig(emb_path='x/emb.npy')
    assert (c.context_len, c.emb_size, c.n_heads, c.qkv_dim, c.bias, c.projection_dim) == (8, 256, 8, 512, False, [32])


def _cspec(V, T, Cc, H, D, proj, K, bias=1):
    from mile_amd import _lib
    cs = _lib.ModelSpecC()
    cs.in_features = T
    widths = list(proj) + [K]
    cs.n_layers = len(widths)
    for i, w in enumerate(widths):
        cs.widths[i] = w
    cs.task, cs.prior, cs.prior_scale, cs.use_bias = 1, 0, 1.0, bias
    cs.model, cs.vocab_size, cs.ctx_len, cs.emb_size, cs.n_heads, cs.qkv_dim = 4, V, T, Cc, H, D
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
    from mile_amd.spec import PretrainedAttentionSpec
    ok = refused = 0
    for T, Cc, H, D, proj in ENVELOPE + [(70, 193, 8, 64, ()), (129, 16, 2, 16, ()), (16, 16, 1, 129, ()),
                                         (16, 16, 2, 16, (129,)), (16, 16, 2, 16, (8, 8, 8))]:
        try:
            spec = PretrainedAttentionSpec(100, T, Cc, H, D, projection_dim=proj, use_bias=True)
            want = True
        except NotImplementedError:
            want = False
        lib, h, rc = _create(_cspec(100, T, Cc, H, D, proj, 2))
        assert (rc == 0) == want, (T, Cc, H, D, proj, rc, lib.mile_last_error())
        if rc == 0:
            assert lib.mile_param_count(h) == spec.n_params
            bo, ko = C.c_int64(), C.c_int64()
            leaves = {n: o for n, o, _ in spec.leaves()}
            for layer, name in enumerate(['MDPA.key', 'MDPA.out', 'MDPA.query', 'MDPA.value', 'classifier']
                                         + [f'projection_{i}' for i in range(len(proj))]):
                assert lib.mile_param_offsets(h, layer, C.byref(bo), C.byref(ko)) == 0
                assert (bo.value, ko.value) == (leaves[f'{name}.bias'], leaves[f'{name}.kernel'])
            assert lib.mile_destroy(h) == 0
            ok += 1
        else:
            refused += 1
    assert ok > 100 and refused > 5
    # both reference shapes run; the stock shape stops fitting past T = 96
    assert PretrainedAttentionSpec(10000, 70, 192, 10, 100, projection_dim=(128, 32)).lds_bytes <= 160 * 1024
    with pytest.raises(NotImplementedError, match='LDS'):
        PretrainedAttentionSpec(10000, 112, 192, 8, 64)


def test_kernel_choice_and_table_calls_without_a_gpu():
    """AUTO resolves to ATTN_PRE_F32 (13), the only kernel model 4 accepts; mile_set_embedding refuses other models."""
    from mile_amd import _lib
    lib, h, rc = _create(_cspec(50, 16, 32, 2, 16, (8,), 2))
    assert rc == 0, lib.mile_last_error()
    try:
        assert lib.mile_get_grad_kernel(h) == _lib.GRAD_KERNEL_IDS['attn_pre_f32'] == 13
        for k in range(1, 14):
            rc = lib.mile_set_grad_kernel(h, k)
            assert (rc == 0) == (k == 13), (k, lib.mile_last_error())
            assert lib.mile_set_grad_kernel(h, 0) == 0
        assert lib.mile_set_grad_kernel(h, 14) == -1
        assert lib.mile_set_embedding(h, None, None, None) == -1
    finally:
        lib.mile_destroy(h)
    cs = _cspec(50, 16, 32, 2, 16, (8,), 2)
    cs.model = 3
    lib, h, rc = _create(cs)
    assert rc == 0
    try:
        buf = (C.c_float * 4)()
        assert lib.mile_set_embedding(h, buf, buf, None) == -1
        assert b'MILE_MODEL_ATTN_PRETRAINED' in lib.mile_last_error()
    finally:
        lib.mile_destroy(h)


def test_table_tool_both_modes(tmp_path):
    """tools/make_embeddings.py (the test name keeps "emb" out of tmp_path, which the path rule would rewrite)."""
    tool = ROOT / 'tools' / 'make_embeddings.py'
    out = tmp_path / 'tabs' / 'emb_large.npy'
    r = subprocess.run([sys.executable, str(tool), '--random', '30', '10', '16', '--seed', '3', '--out', str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info['pos'] == str(tmp_path / 'tabs' / 'pos_emb_large.npy')
    emb, pos = np.load(out), np.load(info['pos'])
    assert emb.shape == (30, 16) and pos.shape == (10, 16) and emb.dtype == np.float32
    assert 0.15 < emb.std() < 0.35                      # 1 / sqrt(16) = 0.25
    # from an AttentionClassifier params file: the two TokenEmbedding_0 leaves
    from mile_amd.spec import AttentionSpec
    full = AttentionSpec(30, 10, 16, 2, 16, projection_dim=(8,))
    flat = np.arange(full.n_params, dtype=np.float32)
    src = tmp_path / 'params_0.npz'
    np.savez_compressed(src, **{n: flat[o:o + int(np.prod(s))].reshape(s) for n, o, s in full.leaves()})
    out2 = tmp_path / 'emb.npy'
    r = subprocess.run([sys.executable, str(tool), '--from', str(src), '--out', str(out2)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    leaves = {n: (o, s) for n, o, s in full.leaves()}
    o, s = leaves['TokenEmbedding_0.Embedding.embedding']
    assert np.array_equal(np.load(out2), flat[o:o + 30 * 16].reshape(s))
    o, s = leaves['TokenEmbedding_0.PositionEmbedding.embedding']
    assert np.array_equal(np.load(tmp_path / 'pos_emb.npy'), flat[o:o + 10 * 16].reshape(s))
