"""AttentionClassifier host side without a GPU: the fp64 restatement tests/attn_ref.py against torch autograd of an
independent restatement, the masking rules, the parameter layout and initialisers, config parsing and the text loader."""
import math
from pathlib import Path

import numpy as np
import pytest

from tests import attn_ref as R

torch = pytest.importorskip('torch')
ROOT = Path(__file__).resolve().parents[1]


def _spec(V=40, T=12, C=16, H=4, D=16, K=3, proj=(8,), bias=True, **kw):
    from mile_amd.spec import AttentionSpec
    return AttentionSpec(V, T, C, H, D, n_classes=K, projection_dim=proj, use_bias=bias, **kw)


def _torch_loglik(spec, theta, x, y):
    """Independent torch restatement (autograd supplies the gradient)."""
    P = {n: theta[o:o + int(np.prod(s))].reshape(s) for n, o, s in spec.leaves()}
    x = torch.as_tensor(x)
    N, T = x.shape
    C, H, D = spec.emb_size, spec.n_heads, spec.qkv_dim
    hd = D // H
    e = P['TokenEmbedding_0.Embedding.embedding'][x] + P['TokenEmbedding_0.PositionEmbedding.embedding'][:T]

    def proj(name):
        out = torch.einsum('ntc,chd->nthd', e, P[f'MDPA.{name}.kernel'])
        return out + P[f'MDPA.{name}.bias'] if spec.use_bias else out

    q, k, v = proj('query') / math.sqrt(hd), proj('key'), proj('value')
    s = torch.einsum('nqhd,nkhd->nhqk', q, k)
    m = (x != 0)
    mask = (m[:, None, :, None] & m[:, None, None, :])
    s = torch.where(mask, s, torch.tensor(torch.finfo(torch.float32).min, dtype=s.dtype))
    p = torch.softmax(s, dim=-1)
    o = torch.einsum('nhqk,nkhd->nqhd', p, v)
    out = torch.einsum('nqhd,hdc->nqc', o, P['MDPA.out.kernel'])
    if spec.use_bias:
        out = out + P['MDPA.out.bias']
    z = out.mean(dim=1)
    for i in range(len(spec.projection_dim)):
        z = z @ P[f'projection_{i}.kernel'] + (P[f'projection_{i}.bias'] if spec.use_bias else 0)
        z = torch.nn.functional.gelu(z, approximate='tanh')
    lg = z @ P['classifier.kernel'] + (P['classifier.bias'] if spec.use_bias else 0)
    return torch.log_softmax(lg, dim=-1)[torch.arange(N), torch.as_tensor(y).long()].sum()


@pytest.mark.parametrize('bias,proj,H,D', [(True, (8,), 4, 16), (False, (6, 5), 2, 16), (True, (), 1, 8), (False, (32,), 8, 64)])
def test_restatement_matches_torch_autograd(bias, proj, H, D):
    spec = _spec(C=16, H=H, D=D, proj=proj, bias=bias)
    prob = R.synthetic_problem(spec, 9, 1, seed=2)
    th = prob['theta0'][0].astype(np.float64)
    ll, g = R.loglik_and_grad(spec, th, prob['x'], prob['y'])
    t = torch.tensor(th, requires_grad=True)
    llt = _torch_loglik(spec, t, prob['x'], prob['y'])
    llt.backward()
    assert abs(ll - llt.item()) < 1e-10 * max(1.0, abs(ll))
    gt = t.grad.numpy()
    assert np.abs(g - gt).max() < 1e-10 * np.abs(gt).max()
    assert np.abs(R.pointwise_loglik(spec, th, prob['x'], prob['y']).sum() - ll) < 1e-10 * max(1.0, abs(ll))


def test_masking_rules():
    spec = _spec(T=8, H=2, D=8, bias=True)
    prob = R.synthetic_problem(spec, 3, 1, seed=5)
    x = np.array([[5, 6, 0, 7, 0, 0, 0, 0],      # a pad id in mid-sequence, then pads
                  [0, 0, 0, 0, 0, 0, 0, 0],      # fully padded
                  [1, 2, 3, 4, 5, 6, 7, 8]])
    y = np.array([0, 1, 2])
    th = prob['theta0'][0].astype(np.float64)
    p = R.attn_probs(spec, R.unpack(spec, th), x)
    real = x != 0
    for n in range(3):
        for i in range(8):
            if real[n, i]:
                assert np.all(p[n, :, i, ~real[n]] == 0.0)          # pad keys of a real query get weight exactly 0
                assert np.allclose(p[n, :, i].sum(-1), 1.0)
            else:
                assert np.allclose(p[n, :, i], 1.0 / 8)             # pad query rows: uniform over all T keys
    # a fully padded sequence has only pad query rows: no gradient reaches q or k, but every v gets some
    t = torch.tensor(th, requires_grad=True)
    ll = _torch_loglik(spec, t, x[1:2], y[1:2])                     # fully padded row: all of its tokens are id 0
    ll.backward()
    g = t.grad.numpy()
    leaves = {n: (o, s) for n, o, s in spec.leaves()}
    for name in ('MDPA.query.kernel', 'MDPA.query.bias', 'MDPA.key.kernel', 'MDPA.key.bias'):
        o, s = leaves[name]
        assert np.all(g[o:o + int(np.prod(s))] == 0.0), name
    o, s = leaves['MDPA.value.kernel']
    assert np.abs(g[o:o + int(np.prod(s))]).max() > 0
    _, gr = R.loglik_and_grad(spec, th, x[1:2], y[1:2])
    assert np.abs(gr - g).max() < 1e-10 * np.abs(g).max()


def test_leaves_order_names_shapes():
    spec = _spec(V=1000, T=70, C=48, H=8, D=64, K=2, proj=(32,), bias=False)
    assert [(n, s) for n, _, s in spec.leaves()] == [
        ('MDPA.key.kernel', (48, 8, 8)), ('MDPA.out.kernel', (8, 8, 48)), ('MDPA.query.kernel', (48, 8, 8)),
        ('MDPA.value.kernel', (48, 8, 8)), ('TokenEmbedding_0.Embedding.embedding', (1000, 48)),
        ('TokenEmbedding_0.PositionEmbedding.embedding', (70, 48)), ('classifier.kernel', (32, 2)),
        ('projection_0.kernel', (48, 32))]
    assert spec.n_params == 4 * 48 * 64 + 1000 * 48 + 70 * 48 + 32 * 2 + 48 * 32
    sb = _spec(V=10, T=5, C=8, H=2, D=8, K=3, proj=(4, 6), bias=True)
    assert [n for n, _, _ in sb.leaves()] == [
        'MDPA.key.bias', 'MDPA.key.kernel', 'MDPA.out.bias', 'MDPA.out.kernel', 'MDPA.query.bias', 'MDPA.query.kernel',
        'MDPA.value.bias', 'MDPA.value.kernel', 'TokenEmbedding_0.Embedding.embedding',
        'TokenEmbedding_0.PositionEmbedding.embedding', 'classifier.bias', 'classifier.kernel', 'projection_0.bias',
        'projection_0.kernel', 'projection_1.bias', 'projection_1.kernel']
    assert dict((n, s) for n, _, s in sb.leaves())['classifier.kernel'] == (6, 3)
    offs = [(o, int(np.prod(s))) for _, o, s in sb.leaves()]
    assert all(a + n == b for (a, n), (b, _) in zip(offs, offs[1:]))
    # the stock shape's FLOP model: 8.93 MFLOP per sequence and chain
    assert abs(spec.flops_per_sequence / 1e6 - 8.93) < 0.01


def test_initialisers():
    from mile_amd.config import Config
    from mile_amd.trainer import BDETrainer
    cfg = Config.from_yaml(ROOT / 'experiments' / 'mclmc_seqmod_synthetic.yaml')
    cfg = cfg.replace(data=cfg.data.__class__(**{**cfg.data.__dict__, 'path': '300x70x1000', 'datapoint_limit': 300}))
    tr = BDETrainer.__new__(BDETrainer)
    tr.config = cfg
    tr.build_model(cfg)
    rows = tr.init_module_params([0, 1, 2, 3])
    spec = tr.prob_model.spec
    L = {n: rows[:, o:o + int(np.prod(s))] for n, o, s in spec.leaves()}
    tn = 0.87962566103423978
    assert abs(L['TokenEmbedding_0.Embedding.embedding'].std() * math.sqrt(48) - 1) < 0.02
    assert abs(L['TokenEmbedding_0.PositionEmbedding.embedding'].std() * math.sqrt(48) - 1) < 0.05
    for name in ('MDPA.query.kernel', 'MDPA.key.kernel', 'MDPA.value.kernel'):     # fan_in = C
        assert abs(L[name].std() * math.sqrt(48) - 1) < 0.05, name
    assert abs(L['MDPA.out.kernel'].std() * math.sqrt(64) - 1) < 0.05                # fan_in = H * hd
    assert np.abs(L['MDPA.query.kernel']).max() <= 2 / math.sqrt(48) / tn + 1e-6
    assert abs(L['projection_0.kernel'].std() * math.sqrt(48) - 1) < 0.05
    assert not np.allclose(rows[0], rows[1])


def test_config_parsing_and_refusals():
    import dataclasses

    from mile_amd.config import AttentionClassifierConfig, Config, ConfigError
    cfg = Config.from_yaml(ROOT / 'experiments' / 'mclmc_seqmod_synthetic.yaml')
    m = cfg.model
    assert isinstance(m, AttentionClassifierConfig)
    assert (m.vocab_size, m.context_len, m.emb_size, m.n_heads, m.qkv_dim, m.bias, m.n_classes, m.projection_dim) == \
        (1000, 70, 48, 8, 64, False, 2, [32])
    assert cfg.training.sampler.n_chains == 8 and cfg.training.sampler.prior_config.parameters['scale'] == 0.2
    ref = {'model', 'vocab_size', 'context_len', 'emb_size', 'n_blocks', 'n_heads', 'qkv_dim', 'bias', 'dropout', 'dtype',
           'n_classes', 'projection_dim'}
    assert {f.name for f in dataclasses.fields(AttentionClassifierConfig)} == ref
    d = AttentionClassifierConfig()
    assert (d.vocab_size, d.context_len, d.emb_size, d.n_blocks, d.n_heads, d.qkv_dim, d.bias, d.dropout, d.n_classes,
            d.projection_dim) == (1000, 8, 256, 6, 8, 512, False, 0.1, 2, [32])
    with pytest.raises(ConfigError, match='bfloat16'):
        AttentionClassifierConfig(dtype='bfloat16')
    with pytest.raises(ConfigError):
        AttentionClassifierConfig(qkv_dim=10, n_heads=3)
    from mile_amd.spec import AttentionSpec
    with pytest.raises(NotImplementedError, match='64'):
        AttentionSpec(1000, 70, 192, 8, 64)                        # the C = 192 pretraining shape
    with pytest.raises(NotImplementedError, match='128'):
        AttentionSpec(1000, 200, 48, 8, 64)
    with pytest.raises(NotImplementedError, match='qkv_dim'):
        AttentionSpec(1000, 70, 48, 10, 100)
    with pytest.raises(NotImplementedError, match='projection'):
        AttentionSpec(1000, 70, 48, 8, 64, projection_dim=(128, 32))
    with pytest.raises(NotImplementedError, match='projection'):
        AttentionSpec(1000, 70, 48, 8, 64, projection_dim=(8, 8, 8))
    with pytest.raises(NotImplementedError, match='n_classes'):
        AttentionSpec(1000, 70, 48, 8, 64, n_classes=17)


def test_text_loader_synthetic_and_npz(tmp_path):
    from mile_amd.config import DataConfig
    from mile_amd.dataset import TextLoader
    dc = DataConfig(path='500x30x100', source='synthetic', data_type='text', task='class', train_split=0.7, valid_split=0.1,
                    test_split=0.2)
    a = TextLoader(dc, rng=7, context_len=30, vocab_size=100)
    b = TextLoader(dc, rng=7, context_len=30, vocab_size=100)
    c = TextLoader(dc, rng=8, context_len=30, vocab_size=100)
    assert np.array_equal(a.train_x, b.train_x) and np.array_equal(a.test_y, b.test_y)
    assert not np.array_equal(a.train_x, c.train_x)
    assert a.train_x.shape == (350, 30) and len(a) == 500 and a.test_x.shape[1] == 30
    x = np.concatenate([a.train_x, a.valid_x, a.test_x]).astype(np.int64)
    assert x.min() == 0 and x.max() < 100
    nz = x != 0                                                    # pads only after the last token
    assert np.all(nz[:, :-1] | ~nz[:, 1:])
    counts = np.bincount(x[nz], minlength=100)
    assert counts[1] > counts[50] > 0                              # Zipf-like frequencies
    y = np.concatenate([a.train_y, a.valid_y, a.test_y])
    assert set(np.unique(y)) == {0, 1}
    np.savez(tmp_path / 't.npz', x=x, y=y)
    dl = DataConfig(path=str(tmp_path / 't.npz'), source='local', data_type='text', task='class', train_split=0.7,
                    valid_split=0.1, test_split=0.2)
    d = TextLoader(dl, rng=1, context_len=30, vocab_size=100)
    assert len(d) == 500
    with pytest.raises(ValueError):
        TextLoader(dl, rng=1, context_len=30, vocab_size=50)
    with pytest.raises(NotImplementedError, match='npz'):
        TextLoader(DataConfig(path='imdb', source='huggingface', data_type='text', task='class', train_split=0.7,
                              valid_split=0.1, test_split=0.2), rng=1, context_len=30, vocab_size=100)


def _attn_cspec(V, T, C, H, D, proj=(32,), K=2, bias=0):
    from mile_amd import _lib
    cs = _lib.ModelSpecC()
    cs.in_features, cs.n_layers = T, len(proj) + 1
    for i, w in enumerate(tuple(proj) + (K,)):
        cs.widths[i] = w
    cs.activation, cs.task, cs.prior, cs.prior_loc, cs.prior_scale, cs.use_bias = 0, 1, 0, 0.0, 0.2, bias
    cs.model, cs.vocab_size, cs.ctx_len, cs.emb_size, cs.n_heads, cs.qkv_dim = 3, V, T, C, H, D
    return cs


def test_spec_and_library_accept_the_same_shapes():
    """AttentionSpec refuses exactly what mile_create refuses (the LDS budget is computed on both sides) over the whole
    C = 64, D <= 64, H | D, T <= 128 envelope, and the library's parameter offsets follow AttentionSpec.leaves()."""
    import ctypes as Cc

    from mile_amd import _lib
    from mile_amd.spec import AttentionSpec
    lib = _lib.load_library()
    h = Cc.c_void_p()
    refused = []
    for D in range(1, 65):
        for H in (H for H in range(1, D + 1) if D % H == 0):
            for T in range(1, 129):
                try:
                    AttentionSpec(50, T, 64, H, D)
                    ok_py = True
                except NotImplementedError as exc:
                    assert 'LDS' in str(exc)
                    ok_py = False
                rc = lib.mile_create(Cc.byref(_attn_cspec(50, T, 64, H, D)), 0, Cc.byref(h))
                assert (rc == 0) == ok_py, (T, H, D, lib.mile_last_error())
                if rc == 0:
                    assert lib.mile_destroy(h) == 0
                else:
                    assert b'LDS' in lib.mile_last_error()
                    refused.append((T, H, D))
    # the one corner the LDS budget excludes: three heads of 19..21 wide with T > 112
    assert sorted({(H, D) for _, H, D in refused}) == [(3, 57), (3, 60), (3, 63)]
    assert min(T for T, _, _ in refused) == 113
    for bias, proj in ((0, (32,)), (1, (6, 5)), (1, ())):
        spec = AttentionSpec(50, 37, 24, 4, 32, n_classes=3, projection_dim=proj, use_bias=bool(bias))
        assert lib.mile_create(Cc.byref(_attn_cspec(50, 37, 24, 4, 32, proj, 3, bias)), 0, Cc.byref(h)) == 0
        assert lib.mile_param_count(h) == spec.n_params
        L = {n: o for n, o, _ in spec.leaves()}
        names = ['MDPA.key', 'MDPA.out', 'MDPA.query', 'MDPA.value', None, None, 'classifier'] + \
            [f'projection_{i}' for i in range(len(proj))]
        for li, nm in enumerate(names):
            b, k = Cc.c_int64(), Cc.c_int64()
            assert lib.mile_param_offsets(h, li, Cc.byref(b), Cc.byref(k)) == 0
            if nm is None:
                assert k.value == L['TokenEmbedding_0.Embedding.embedding' if li == 4 else
                                    'TokenEmbedding_0.PositionEmbedding.embedding'] and b.value == -1
            else:
                assert k.value == L[f'{nm}.kernel'] and b.value == (L[f'{nm}.bias'] if bias else -1), nm
        assert lib.mile_destroy(h) == 0
