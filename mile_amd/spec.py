"""Model spec and raveled-parameter layout of the FCN target.

Mirrors what the reference's closure ``partial(log_unnormalized_posterior, x=..., y=...)``
captures (src/training/trainer.py:576-580): FCNConfig (src/config/models/fcn.py:7-30),
the prior (src/training/priors.py:67-91) and the task (src/training/probabilistic.py:92-109).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

ACTIVATIONS = ('relu', 'tanh', 'sigmoid')
TASKS = ('regr', 'classification')
PRIORS = ('Normal', 'StandardNormal', 'Laplace')


@dataclass(frozen=True)
class ModelSpec:
    """``hidden_structure`` as in FCNConfig: one entry per Dense layer, last = output layer."""

    in_features: int
    hidden_structure: tuple
    activation: str = 'relu'
    task: str = 'regr'
    prior: str = 'StandardNormal'
    prior_loc: float = 0.0
    prior_scale: float = 1.0
    use_bias: bool = True
    root: str = 'fcn'   # name of the FullyConnected submodule inside FCN (src/models/tabular/fcn.py:18)

    def __post_init__(self):
        object.__setattr__(self, 'hidden_structure', tuple(int(w) for w in self.hidden_structure))
        if self.activation not in ACTIVATIONS:
            raise NotImplementedError(f'activation {self.activation!r} (supported: {ACTIVATIONS})')
        if self.task not in TASKS:
            raise NotImplementedError(f'Likelihood computation for {self.task} not implemented')
        if self.prior not in PRIORS:
            raise NotImplementedError(f'Prior Distribution for {self.prior} is not yet implemented.')
        if self.prior == 'StandardNormal':
            object.__setattr__(self, 'prior_loc', 0.0)
            object.__setattr__(self, 'prior_scale', 1.0)
        if self.task == 'regr' and self.hidden_structure[-1] != 2:
            raise ValueError('regression needs hidden_structure[-1] == 2 (mu, log sigma)')

    @property
    def layer_dims(self):
        dims, fin = [], self.in_features
        for w in self.hidden_structure:
            dims.append((fin, w))
            fin = w
        return dims

    @property
    def n_params(self) -> int:
        return sum(i * o + (o if self.use_bias else 0) for i, o in self.layer_dims)

    def layer_order(self):
        """ravel_pytree visits dict keys sorted as strings: 'layer10' < 'layer2'."""
        return sorted(range(len(self.hidden_structure)), key=lambda i: f'layer{i}')

    def leaves(self):
        """[(dotted name, offset, shape)] in pytree order == np.savez key order of
        save_position (src/training/callbacks.py:36-43, src/utils.py:50-70)."""
        out, off = [], 0
        for li in self.layer_order():
            fin, fout = self.layer_dims[li]
            if self.use_bias:
                out.append((f'{self.root}.layer{li}.bias', off, (fout,)))
                off += fout
            out.append((f'{self.root}.layer{li}.kernel', off, (fin, fout)))
            off += fin * fout
        return out


@dataclass(frozen=True)
class LeNetSpec:
    """LeNet (src/models/images/cnns.py:10-66, LeNetConfig src/config/models/cnns.py) on [N, C, H, W] images:
    Conv(6, 5x5, pad 2) - act - avg_pool 2 - Conv(16, 5x5) - act - avg_pool 2 - Dense 120 - Dense 84 - Dense out_dim.
    Duck-types ModelSpec where the host code needs it (in_features, n_params, leaves, task/prior fields)."""

    channels: int
    height: int
    width: int
    out_dim: int
    activation: str = 'relu'
    task: str = 'classification'
    prior: str = 'StandardNormal'
    prior_loc: float = 0.0
    prior_scale: float = 1.0
    use_bias: bool = True
    root: str = 'core'   # name of the LeNetCore submodule inside LeNet (cnns.py:21-25)

    def __post_init__(self):
        if self.activation not in ACTIVATIONS:
            raise NotImplementedError(f'activation {self.activation!r} (supported: {ACTIVATIONS})')
        if self.task not in TASKS:
            raise NotImplementedError(f'Likelihood computation for {self.task} not implemented')
        if self.prior not in PRIORS:
            raise NotImplementedError(f'Prior Distribution for {self.prior} is not yet implemented.')
        if self.prior == 'StandardNormal':
            object.__setattr__(self, 'prior_loc', 0.0)
            object.__setattr__(self, 'prior_scale', 1.0)
        if not self.use_bias:
            raise NotImplementedError('use_bias=False is not supported')
        if self.task == 'regr' and self.out_dim != 2:
            raise ValueError('regression needs out_dim == 2 (mu, log sigma)')
        if (self.height // 2 - 4) // 2 < 1 or (self.width // 2 - 4) // 2 < 1:
            raise ValueError('image too small for LeNet')

    @property
    def in_features(self) -> int:
        return self.channels * self.height * self.width

    @property
    def flat(self) -> int:
        return ((self.height // 2 - 4) // 2) * ((self.width // 2 - 4) // 2) * 16

    @property
    def hidden_structure(self):          # only its last entry (the output width) is meaningful for LeNet
        return (self.out_dim,)

    def leaves(self):
        """[(dotted name, offset, shape)] in ravel_pytree order: conv1, conv2, fc1, fc2, fc3; bias before kernel;
        conv kernels [kh, kw, in, out] as flax stores them."""
        shapes = [('conv1.bias', (6,)), ('conv1.kernel', (5, 5, self.channels, 6)),
                  ('conv2.bias', (16,)), ('conv2.kernel', (5, 5, 6, 16)),
                  ('fc1.bias', (120,)), ('fc1.kernel', (self.flat, 120)),
                  ('fc2.bias', (84,)), ('fc2.kernel', (120, 84)),
                  ('fc3.bias', (self.out_dim,)), ('fc3.kernel', (84, self.out_dim))]
        out, off = [], 0
        for name, sh in shapes:
            out.append((f'{self.root}.{name}', off, sh))
            n = 1
            for v in sh:
                n *= v
            off += n
        return out

    @property
    def n_params(self) -> int:
        name, off, sh = self.leaves()[-1]
        n = 1
        for v in sh:
            n *= v
        return off + n


# geometry the LeNetti kernel (mile_amd/csrc/mile_lenetti.h) supports
LENETTI_MAX_CHANNELS = 4
LENETTI_MAX_PIXELS = 2048      # conv-output pixels (H+2)(W+2)
LENETTI_MAX_OUT = 16


@dataclass(frozen=True)
class LeNettiSpec:
    """LeNetti (src/models/images/cnns.py:69-121, LeNettiConfig src/config/models/cnns.py) on [N, C, H, W] images:
    Conv(1, 3x3, pad 2) - act - flatten ((H+2)(W+2) features) - Dense 8 - act - Dense 8 - act - Dense 8 - act - Dense out_dim.
    Duck-types ModelSpec where the host code needs it, as LeNetSpec does."""

    channels: int
    height: int
    width: int
    out_dim: int
    activation: str = 'sigmoid'
    task: str = 'classification'
    prior: str = 'StandardNormal'
    prior_loc: float = 0.0
    prior_scale: float = 1.0
    use_bias: bool = True
    root: str = 'core'   # name of the LeNettiCore submodule inside LeNetti (LeNetti.setup)

    def __post_init__(self):
        if self.activation not in ACTIVATIONS:
            raise NotImplementedError(f'activation {self.activation!r} (supported: {ACTIVATIONS})')
        if self.task not in TASKS:
            raise NotImplementedError(f'Likelihood computation for {self.task} not implemented')
        if self.prior not in PRIORS:
            raise NotImplementedError(f'Prior Distribution for {self.prior} is not yet implemented.')
        if self.prior == 'StandardNormal':
            object.__setattr__(self, 'prior_loc', 0.0)
            object.__setattr__(self, 'prior_scale', 1.0)
        if not self.use_bias:
            raise NotImplementedError('use_bias=False is not supported')
        if self.task == 'regr' and self.out_dim != 2:
            raise ValueError('regression needs out_dim == 2 (mu, log sigma)')
        if min(self.channels, self.height, self.width, self.out_dim) < 1:
            raise ValueError('LeNetti: channels, height, width and out_dim must be >= 1')
        if self.channels > LENETTI_MAX_CHANNELS:
            raise NotImplementedError(f'LeNetti: at most {LENETTI_MAX_CHANNELS} image channels on the HIP kernel')
        if self.pixels > LENETTI_MAX_PIXELS:
            raise NotImplementedError(f'LeNetti: (H+2)*(W+2) = {self.pixels} conv-output pixels, the HIP kernel takes at most '
                                      f'{LENETTI_MAX_PIXELS}')
        if self.out_dim > LENETTI_MAX_OUT:
            raise NotImplementedError(f'LeNetti: out_dim <= {LENETTI_MAX_OUT} on the HIP kernel')

    @property
    def in_features(self) -> int:
        return self.channels * self.height * self.width

    @property
    def pixels(self) -> int:
        """P: features after the flatten, one per conv-output pixel (one output channel)."""
        return (self.height + 2) * (self.width + 2)

    @property
    def hidden_structure(self):          # only its last entry (the output width) is meaningful for LeNetti
        return (self.out_dim,)

    def leaves(self):
        """[(dotted name, offset, shape)] in ravel_pytree order: conv1, fc1, fc2, fc3, fc4; bias before kernel;
        the conv kernel [kh, kw, in, out] as flax stores it."""
        shapes = [('conv1.bias', (1,)), ('conv1.kernel', (3, 3, self.channels, 1)),
                  ('fc1.bias', (8,)), ('fc1.kernel', (self.pixels, 8)),
                  ('fc2.bias', (8,)), ('fc2.kernel', (8, 8)),
                  ('fc3.bias', (8,)), ('fc3.kernel', (8, 8)),
                  ('fc4.bias', (self.out_dim,)), ('fc4.kernel', (8, self.out_dim))]
        out, off = [], 0
        for name, sh in shapes:
            out.append((f'{self.root}.{name}', off, sh))
            n = 1
            for v in sh:
                n *= v
            off += n
        return out

    @property
    def n_params(self) -> int:
        name, off, sh = self.leaves()[-1]
        n = 1
        for v in sh:
            n *= v
        return off + n


IMAGE_SPECS = (LeNetSpec, LeNettiSpec)


# shapes the AttentionClassifier kernel (mile_amd/csrc/mile_attn.h) supports
ATTN_MAX_T = 128
ATTN_MAX_C = 64
ATTN_MAX_D = 64
ATTN_MAX_PROJ = 2
ATTN_MAX_P = 64
ATTN_MAX_K = 16
ATTN_LDS_MAX = 160 * 1024


def attn_lds_bytes(T: int, C: int, H: int, D: int, weights: bool) -> int:
    """LDS of one k_grad_attn workgroup (attn_lds_bytes in mile_attn.h)."""
    Tp, hd = (T + 15) // 16 * 16, D // H
    per_wave = 16 * Tp + (Tp * ((hd + 15) // 16 * 16) if hd > 16 else 0)
    scr = max(64 * Tp, min(H, 4) * per_wave)
    return 4 * ((C * 3 * D if weights else 0) + Tp * 3 * D + scr + 5 * Tp + 10 * 64 + 16)


@dataclass(frozen=True)
class AttentionSpec:
    """AttentionClassifier (src/models/text/attention_classifier.py, AttentionClassifierConfig src/config/models/gpt.py) on
    [N, T] token ids (pad id 0): TokenEmbedding (token + position) - one MultiHeadDotProductAttention 'MDPA' (H heads, qkv_dim D,
    out_features C) - mean over the T positions - (Dense P_i - gelu) per projection - Dense n_classes 'classifier'.
    Duck-types ModelSpec where the host code needs it (in_features = T, hidden_structure = projection_dim + [n_classes])."""

    vocab_size: int
    context_len: int
    emb_size: int
    n_heads: int
    qkv_dim: int
    n_classes: int = 2
    projection_dim: tuple = (32,)
    use_bias: bool = False
    activation: str = 'relu'          # unused: the projections use gelu; kept for the ModelSpec interface
    task: str = 'classification'
    prior: str = 'StandardNormal'
    prior_loc: float = 0.0
    prior_scale: float = 1.0
    root: str = ''

    def __post_init__(self):
        object.__setattr__(self, 'projection_dim', tuple(int(p) for p in self.projection_dim))
        if self.task != 'classification':
            raise NotImplementedError('AttentionClassifier: classification only')
        if self.prior not in PRIORS:
            raise NotImplementedError(f'Prior Distribution for {self.prior} is not yet implemented.')
        if self.prior == 'StandardNormal':
            object.__setattr__(self, 'prior_loc', 0.0)
            object.__setattr__(self, 'prior_scale', 1.0)
        V, T, C, H, D, K = self.vocab_size, self.context_len, self.emb_size, self.n_heads, self.qkv_dim, self.n_classes
        if min(V, T, C, H, D, K) < 1 or any(p < 1 for p in self.projection_dim):
            raise ValueError('AttentionClassifier: all sizes must be >= 1')
        if D % H:
            raise ValueError(f'AttentionClassifier: n_heads ({H}) must divide qkv_dim ({D})')
        if T > ATTN_MAX_T:
            raise NotImplementedError(f'AttentionClassifier: context_len = {T}, the HIP kernel takes at most {ATTN_MAX_T}')
        if C > ATTN_MAX_C:
            raise NotImplementedError(f'AttentionClassifier: emb_size = {C}, the HIP kernel takes at most {ATTN_MAX_C} '
                                      '(its weights must fit on chip)')
        if D > ATTN_MAX_D:
            raise NotImplementedError(f'AttentionClassifier: qkv_dim = {D}, the HIP kernel takes at most {ATTN_MAX_D}')
        if len(self.projection_dim) > ATTN_MAX_PROJ:
            raise NotImplementedError(f'AttentionClassifier: at most {ATTN_MAX_PROJ} projection layers on the HIP kernel')
        if any(p > ATTN_MAX_P for p in self.projection_dim):
            raise NotImplementedError(f'AttentionClassifier: projection widths <= {ATTN_MAX_P} on the HIP kernel')
        if K > ATTN_MAX_K:
            raise NotImplementedError(f'AttentionClassifier: n_classes <= {ATTN_MAX_K} on the HIP kernel')
        if V >= 1 << 24:
            raise NotImplementedError('AttentionClassifier: vocab_size < 2^24 (token ids travel as fp32)')
        if attn_lds_bytes(T, C, H, D, False) > ATTN_LDS_MAX:
            raise NotImplementedError(f'AttentionClassifier: this shape needs more than {ATTN_LDS_MAX // 1024} KB of LDS '
                                      'per workgroup on the HIP kernel')

    @property
    def in_features(self) -> int:
        return self.context_len

    @property
    def head_dim(self) -> int:
        return self.qkv_dim // self.n_heads

    @property
    def hidden_structure(self):
        return self.projection_dim + (self.n_classes,)

    def leaves(self):
        """[(dotted name, offset, shape)] in ravel_pytree order: sorted keys at every level (uppercase before lowercase),
        bias before kernel; biases only with use_bias.  DenseGeneral kernels keep flax's [C, H, hd] / [H, hd, C] shapes."""
        C, H, hd, D, K = self.emb_size, self.n_heads, self.head_dim, self.qkv_dim, self.n_classes
        shapes = []

        def dense(name, bias_shape, kernel_shape):
            if self.use_bias:
                shapes.append((f'{name}.bias', bias_shape))
            shapes.append((f'{name}.kernel', kernel_shape))

        dense('MDPA.key', (H, hd), (C, H, hd))
        dense('MDPA.out', (C,), (H, hd, C))
        dense('MDPA.query', (H, hd), (C, H, hd))
        dense('MDPA.value', (H, hd), (C, H, hd))
        shapes.append(('TokenEmbedding_0.Embedding.embedding', (self.vocab_size, C)))
        shapes.append(('TokenEmbedding_0.PositionEmbedding.embedding', (self.context_len, C)))
        dense('classifier', (K,), ((self.projection_dim[-1] if self.projection_dim else C), K))
        fin = C
        for i, p in enumerate(self.projection_dim):
            dense(f'projection_{i}', (p,), (fin, p))
            fin = p
        out, off = [], 0
        for name, sh in shapes:
            out.append((f'{self.root}.{name}' if self.root else name, off, sh))
            n = 1
            for v in sh:
                n *= v
            off += n
        return out

    @property
    def n_params(self) -> int:
        name, off, sh = self.leaves()[-1]
        n = 1
        for v in sh:
            n *= v
        return off + n

    @property
    def lds_bytes(self) -> int:
        """LDS of one k_grad_attn workgroup: with Wq|Wk|Wv staged when they fit, without them otherwise."""
        args = (self.context_len, self.emb_size, self.n_heads, self.qkv_dim)
        with_w = attn_lds_bytes(*args, True)
        return with_w if with_w <= ATTN_LDS_MAX else attn_lds_bytes(*args, False)

    @property
    def flops_per_sequence(self) -> int:
        """3 x forward: 2 T C 3D + 4 T^2 D + 2 T D C + sum 2 P_{i-1} P_i (projections and classifier)."""
        T, C, D = self.context_len, self.emb_size, self.qkv_dim
        dims = (C,) + self.hidden_structure
        fwd = 2 * T * C * 3 * D + 4 * T * T * D + 2 * T * D * C + sum(2 * a * b for a, b in zip(dims[:-1], dims[1:]))
        return 3 * fwd



# shapes the PretrainedAttentionClassifier kernel (mile_amd/csrc/mile_attn_pre.h) supports
ATTNP_MAX_C = 192
ATTNP_MAX_D = 128
ATTNP_MAX_P = 128


def attn_pre_lds_bytes(T: int, C: int, H: int, D: int, projection_dim=()) -> int:
    """LDS of one k_grad_attn_pre workgroup (attnp_lds_bytes in mile_attn_pre.h): q|k|v [Tp][3D], a scratch that holds
    e [Tp][C] or the busy waves' dS | u | dK, and the tail vectors."""
    Tp, hd = (T + 15) // 16 * 16, D // H
    P = tuple(projection_dim)
    per_wave = 17 * Tp + (Tp * ((hd + 15) // 16 * 16) if hd > 16 else 0)
    scr = max(Tp * C, min(H, 4) * per_wave)
    W = max((C,) + P)
    vec = Tp + 2 * D + C + 2 * sum(P) + (P[-1] if P else C) + 2 * W + 16
    return 4 * (Tp * 3 * D + scr + vec)


def pretrained_table_paths(emb_path) -> tuple[str, str]:
    """The token table's path and the position table's: PretrainedTokenEmbedding's plain str.replace('emb', 'pos_emb')
    over the WHOLE path (src/flax_building_blocks/basic.py:129-135), so every 'emb' in it is rewritten, directories included:
    'results/emb.npy' -> 'results/pos_emb.npy', 'emb_large.npy' -> 'pos_emb_large.npy'."""
    emb_path = str(emb_path)
    return emb_path, emb_path.replace('emb', 'pos_emb')


def _check_streamed_attention(self, name: str):
    """__post_init__ of the two specs on the kernel that streams its weights (mile_attn_pre.h's body): PretrainedAttentionSpec and
    WideAttentionSpec share its limits and its LDS budget."""
    object.__setattr__(self, 'projection_dim', tuple(int(p) for p in self.projection_dim))
    if self.task != 'classification':
        raise NotImplementedError(f'{name}: classification only')
    if self.prior not in PRIORS:
        raise NotImplementedError(f'Prior Distribution for {self.prior} is not yet implemented.')
    if self.prior == 'StandardNormal':
        object.__setattr__(self, 'prior_loc', 0.0)
        object.__setattr__(self, 'prior_scale', 1.0)
    V, T, C, H, D, K = self.vocab_size, self.context_len, self.emb_size, self.n_heads, self.qkv_dim, self.n_classes
    if min(V, T, C, H, D, K) < 1 or any(p < 1 for p in self.projection_dim):
        raise ValueError(f'{name}: all sizes must be >= 1')
    if D % H:
        raise ValueError(f'{name}: n_heads ({H}) must divide qkv_dim ({D})')
    limits = ((T, ATTN_MAX_T, 'context_len'), (C, ATTNP_MAX_C, 'emb_size'), (D, ATTNP_MAX_D, 'qkv_dim'),
              (K, ATTN_MAX_K, 'n_classes'))
    for v, top, what in limits:
        if v > top:
            raise NotImplementedError(f'{name}: {what} = {v}, the HIP kernel takes at most {top}')
    if len(self.projection_dim) > ATTN_MAX_PROJ:
        raise NotImplementedError(f'{name}: at most {ATTN_MAX_PROJ} projection layers on the HIP kernel')
    if any(p > ATTNP_MAX_P for p in self.projection_dim):
        raise NotImplementedError(f'{name}: projection widths <= {ATTNP_MAX_P} on the HIP kernel')
    if V >= 1 << 24:
        raise NotImplementedError(f'{name}: vocab_size < 2^24 (token ids travel as fp32)')
    if self.lds_bytes > ATTN_LDS_MAX:
        raise NotImplementedError(f'{name}: this shape needs {self.lds_bytes} bytes of LDS per workgroup, the HIP kernel '
                                  f'has {ATTN_LDS_MAX} (q|k|v [T][3D] and e [T][C] share it)')


@dataclass(frozen=True)
class PretrainedAttentionSpec:
    """PretrainedAttentionClassifier (src/models/text/attention_classifier.py:74-132, PretrainedAttentionClassifierConfig
    src/config/models/gpt.py:55-61) on [N, T] token ids (pad id 0): e = emb[x] + pos[0..T) from frozen tables (`emb_path` and
    its pos_emb twin, see pretrained_table_paths) - MultiHeadDotProductAttention 'MDPA' - mean over the T positions -
    (Dense P_i - gelu) per projection - gelu - Dense n_classes 'classifier'.  The tables are not parameters: they are neither
    sampled nor in the prior.  Duck-types ModelSpec as AttentionSpec does."""

    vocab_size: int
    context_len: int
    emb_size: int
    n_heads: int
    qkv_dim: int
    n_classes: int = 2
    projection_dim: tuple = (32,)
    use_bias: bool = False
    emb_path: str | None = None
    activation: str = 'relu'          # unused: the projections use gelu; kept for the ModelSpec interface
    task: str = 'classification'
    prior: str = 'StandardNormal'
    prior_loc: float = 0.0
    prior_scale: float = 1.0
    root: str = ''

    def __post_init__(self):
        _check_streamed_attention(self, 'PretrainedAttentionClassifier')

    @property
    def in_features(self) -> int:
        return self.context_len

    @property
    def head_dim(self) -> int:
        return self.qkv_dim // self.n_heads

    @property
    def hidden_structure(self):
        return self.projection_dim + (self.n_classes,)

    def leaves(self):
        """[(dotted name, offset, shape)] in ravel_pytree order: AttentionSpec's without the TokenEmbedding_0 tables."""
        full = AttentionSpec.leaves(self)
        out, off = [], 0
        for name, _, sh in full:
            if 'TokenEmbedding_0.' in name:
                continue
            out.append((name, off, sh))
            off += int(np.prod(sh))
        return out

    @property
    def n_params(self) -> int:
        name, off, sh = self.leaves()[-1]
        return off + int(np.prod(sh))

    @property
    def lds_bytes(self) -> int:
        return attn_pre_lds_bytes(self.context_len, self.emb_size, self.n_heads, self.qkv_dim, self.projection_dim)

    @property
    def flops_per_sequence(self) -> int:
        """3 x AttentionSpec's forward, minus the 2 T C 3D input-gradient product a frozen table does not need."""
        T, C, D = self.context_len, self.emb_size, self.qkv_dim
        dims = (C,) + self.hidden_structure
        fwd = 2 * T * C * 3 * D + 4 * T * T * D + 2 * T * D * C + sum(2 * a * b for a, b in zip(dims[:-1], dims[1:]))
        return 3 * fwd - 2 * T * C * 3 * D

    def table_paths(self) -> tuple[str, str]:
        if not self.emb_path:
            raise ValueError('PretrainedAttentionClassifier needs emb_path (the .npy token table; tools/make_embeddings.py '
                             'writes one)')
        return pretrained_table_paths(self.emb_path)

    def check_tables(self, emb, pos) -> tuple[np.ndarray, np.ndarray]:
        """emb [V, C] and the first T rows of pos [>= T, C], as contiguous fp32 arrays."""
        V, T, C = self.vocab_size, self.context_len, self.emb_size
        emb = np.ascontiguousarray(np.asarray(emb), dtype=np.float32)
        pos = np.asarray(pos)
        if emb.shape != (V, C):
            raise ValueError(f'embedding table: expected [vocab_size, emb_size] = [{V}, {C}], got {list(emb.shape)}')
        if pos.ndim != 2 or pos.shape[0] < T or pos.shape[1] != C:
            raise ValueError(f'position table: expected at least {T} rows (context_len) of emb_size = {C}, got {list(pos.shape)}')
        if not (np.isfinite(emb).all() and np.isfinite(pos[:T]).all()):
            raise ValueError('embedding tables must be finite')
        return emb, np.ascontiguousarray(pos[:T], dtype=np.float32)

    def load_tables(self) -> tuple[np.ndarray, np.ndarray]:
        """The one loader: np.load of both paths (pretrained_table_paths), validated and cast by check_tables."""
        emb_path, pos_path = self.table_paths()
        tables = []
        for what, path in (('embedding', emb_path), ('position', pos_path)):
            try:
                tables.append(np.load(path))
            except FileNotFoundError as exc:
                raise FileNotFoundError(f'{what} table {path!r} not found (emb_path {self.emb_path!r}; tools/make_embeddings.py '
                                        'writes both tables)') from exc
        return self.check_tables(*tables)


@dataclass(frozen=True)
class WideAttentionSpec(AttentionSpec):
    """AttentionClassifier beyond the on-chip kernel's widths: the model, fields, leaves and FLOP model of AttentionSpec, the
    limits and LDS of the kernel that streams its weights (k_grad_attn_wide, mile_amd/csrc/mile_attn_wide.h: emb_size <= 192,
    qkv_dim <= 128, projections <= 128 -- the reference's emb_size-192 pretraining shapes).  The embedding tables are
    parameters: 4 V C bytes of every slab row (see slab_bytes)."""

    def __post_init__(self):
        _check_streamed_attention(self, 'AttentionClassifier (wide kernel)')

    @property
    def lds_bytes(self) -> int:
        """LDS of one k_grad_attn_wide workgroup (attnp_lds_bytes in mile_attn_pre.h): the pretrained kernel's."""
        return attn_pre_lds_bytes(self.context_len, self.emb_size, self.n_heads, self.qkv_dim, self.projection_dim)

    def row_splits(self, n_chains: int, n_rows: int, n_cu: int = 256) -> int:
        """Row ranges (slab rows) per chain of k_grad_attn_wide (attn_wide_S in mile_hip.hip): one workgroup per CU, at least 8
        sequences per range, no cap."""
        want = (n_cu + max(n_chains, 1) - 1) // max(n_chains, 1)
        return max(1, min(want, max(1, n_rows // 8)))

    def slab_bytes(self, n_chains: int, n_rows: int, n_cu: int = 256) -> int:
        """Bytes of the [E, S, d] gradient slabs mile_reserve allocates for n_chains on n_rows (Engine.slab_bytes is what the
        library holds; tests/test_gpu_attn_wide.py holds the two equal)."""
        return 4 * n_chains * self.row_splits(n_chains, n_rows, n_cu) * ((self.n_params + 3) // 4 * 4)


def attention_spec(**kw):
    """The spec of `model: AttentionClassifier`: AttentionSpec (the on-chip k_grad_attn) wherever it takes the shape, so no shape
    that ran before changes kernel; WideAttentionSpec (k_grad_attn_wide) beyond it."""
    try:
        return AttentionSpec(**kw)
    except NotImplementedError:
        return WideAttentionSpec(**kw)


NATIVE_SPECS = IMAGE_SPECS + (AttentionSpec, PretrainedAttentionSpec, WideAttentionSpec)
