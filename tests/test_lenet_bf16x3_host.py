"""Host side of the `lenet_bf16x3` grad kernel (MILE_GRAD_LENET_BF16X3 = 15; no GPU): which specs mile_set_grad_kernel
accepts it for, that AUTO still resolves LeNet to LENET_F32, and the Python / YAML surface.  (The three-term split is
device code -- mm_split4 -- with no host-side form, so it is checked on the GPU through the gradient bounds only.)"""
import ctypes as C
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

X3 = 15


def _cspec(F, widths, task=0):
    from mile_amd import _lib
    cs = _lib.ModelSpecC()
    cs.in_features, cs.n_layers = F, len(widths)
    for i, w in enumerate(widths):
        cs.widths[i] = w
    cs.activation, cs.task, cs.prior, cs.prior_loc, cs.prior_scale, cs.use_bias = 0, task, 0, 0.0, 1.0, 1
    return cs


def _image(model, c, h, w, k):
    cs = _cspec(c * h * w, (k,), task=1)
    cs.model, cs.img_c, cs.img_h, cs.img_w = model, c, h, w
    return cs


def _attn(model):
    cs = _cspec(16, (3,), task=1)
    cs.model, cs.vocab_size, cs.ctx_len, cs.emb_size, cs.n_heads, cs.qkv_dim = model, 50, 16, 16, 2, 16
    return cs


def _handle(cs):
    from mile_amd import _lib
    lib = _lib.load_library()
    h = C.c_void_p()
    assert lib.mile_create(C.byref(cs), 0, C.byref(h)) == 0, lib.mile_last_error()
    return lib, h


def test_id_15_is_a_lenet_kernel_and_auto_is_unchanged():
    from mile_amd import _lib
    assert _lib.GRAD_KERNEL_IDS['lenet_bf16x3'] == X3 and _lib.ABI_VERSION == 10
    lib, h = _handle(_image(1, 1, 28, 28, 10))
    try:
        assert lib.mile_get_grad_kernel(h) == 5                      # AUTO: LENET_F32
        assert lib.mile_set_grad_kernel(h, X3) == 0, lib.mile_last_error()
        assert lib.mile_get_grad_kernel(h) == X3
        assert lib.mile_set_grad_kernel(h, 0) == 0
        assert lib.mile_get_grad_kernel(h) == 5                      # and AUTO again
        assert lib.mile_set_grad_kernel(h, 16) == -1 and lib.mile_last_error()
        assert lib.mile_get_grad_kernel(h) == 5
    finally:
        assert lib.mile_destroy(h) == 0


@pytest.mark.parametrize('name,make', [
    ('lenet_c5', lambda: _image(1, 5, 16, 16, 10)),                  # more than 4 image channels: one slot per pixel no longer
    ('fcn', lambda: _cspec(5, (64, 64, 2))),
    ('lenetti', lambda: _image(2, 1, 8, 8, 3)),
    ('attn', lambda: _attn(3)),
    ('attn_pretrained', lambda: _attn(4)),
    ('attn_wide', lambda: _attn(5)),
])
def test_id_15_is_refused_for_every_other_spec(name, make):
    lib, h = _handle(make())
    try:
        auto = lib.mile_get_grad_kernel(h)
        assert lib.mile_set_grad_kernel(h, X3) == -1, name
        assert b'LENET_BF16X3' in lib.mile_last_error()
        assert lib.mile_get_grad_kernel(h) == auto                   # a refusal leaves the choice as it was
    finally:
        assert lib.mile_destroy(h) == 0


def test_yaml_and_warmstart_surface():
    import yaml
    from mile_amd import warmstart
    from mile_amd.config import Config, ConfigError
    d = yaml.safe_load((ROOT / 'experiments' / 'mclmc_cifar_lenet_b5.yaml').read_text())
    d['training']['sampler']['grad_kernel'] = 'lenet_bf16x3'
    assert Config.from_dict(d).training.sampler.grad_kernel == 'lenet_bf16x3'
    d['training']['sampler']['grad_kernel'] = 'lenet_bf16x4'
    with pytest.raises(ConfigError, match='grad_kernel'):
        Config.from_dict(d)
    assert 'lenet_bf16x3' in warmstart.WINDOWED and 'lenet_bf16' in warmstart.WINDOWED
    assert 'mfma_w128_bf16' not in warmstart.WINDOWED and 'gemm_f32' not in warmstart.WINDOWED
