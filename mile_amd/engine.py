"""Thin torch <-> C-ABI shim around libmile_hip.so.

PyTorch-ROCm is plumbing here: it owns device memory and the stream; every compute
call goes through the C ABI of include/mile_hip.h on raw device pointers.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import torch

from mile_amd import _lib
from mile_amd.spec import (IMAGE_SPECS, AttentionSpec, LeNetSpec, LeNettiSpec, ModelSpec, PretrainedAttentionSpec,
                           WideAttentionSpec)


class IntegratorState(NamedTuple):
    """blackjax IntegratorState with a leading ensemble axis (one row per chain)."""

    position: torch.Tensor         # [E, d]
    momentum: torch.Tensor         # [E, d]
    logdensity: torch.Tensor       # [E]
    logdensity_grad: torch.Tensor  # [E, d]


class MCLMCInfo(NamedTuple):
    """blackjax MCLMCInfo, [n_steps, E] each."""

    logdensity: torch.Tensor
    kinetic_change: torch.Tensor
    energy_change: torch.Tensor


class HMCState(NamedTuple):
    """blackjax HMCState with a leading ensemble axis."""

    position: torch.Tensor         # [E, d]
    logdensity: torch.Tensor       # [E]
    logdensity_grad: torch.Tensor  # [E, d]


class NUTSInfo(NamedTuple):
    """The NUTSInfo fields the reference keeps (src/training/sampling.py:200-210), [n_steps, E] each."""

    num_integration_steps: torch.Tensor
    acceptance_rate: torch.Tensor
    num_trajectory_expansions: torch.Tensor
    is_divergent: torch.Tensor
    energy: torch.Tensor
    is_turning: torch.Tensor


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _f32(t, device, shape=None, name='tensor'):
    t = torch.as_tensor(t, device=device)
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    t = t.contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}')
    return t



def _check_tokens(spec, X):
    """AttentionClassifier rows are token ids stored as fp32: integers in [0, vocab_size)."""
    if not isinstance(spec, (AttentionSpec, PretrainedAttentionSpec)) or not X.numel():
        return
    if bool((X != torch.floor(X)).any()) or float(X.min()) < 0 or float(X.max()) >= spec.vocab_size:
        raise ValueError(f'token ids must be integers in [0, {spec.vocab_size})')


class Engine:
    """One handle == one device, one model spec, one training set."""

    def __init__(self, spec: ModelSpec, X, y, device=None, grad_kernel: str = 'auto', tables=None):
        """tables: (emb, pos) of a PretrainedAttentionSpec; None loads them from spec.emb_path (spec.load_tables)."""
        if not torch.cuda.is_available():
            raise _lib.MileHipError('mile_amd needs an MI355X (torch.cuda.is_available() is False); '
                                    'there is no CPU fallback.')
        self.lib = _lib.load_library()
        self.spec = spec
        self.device = torch.device(device if device is not None else f'cuda:{torch.cuda.current_device()}')
        cs = _lib.ModelSpecC()
        cs.in_features = spec.in_features
        if isinstance(spec, IMAGE_SPECS):
            cs.model = 2 if isinstance(spec, LeNettiSpec) else 1
            cs.img_c, cs.img_h, cs.img_w = spec.channels, spec.height, spec.width
        if isinstance(spec, (AttentionSpec, PretrainedAttentionSpec)):
            cs.model = _lib.MODEL_IDS['attn_pretrained' if isinstance(spec, PretrainedAttentionSpec) else
                                      ('attn_wide' if isinstance(spec, WideAttentionSpec) else 'attn')]
            cs.vocab_size, cs.ctx_len, cs.emb_size = spec.vocab_size, spec.context_len, spec.emb_size
            cs.n_heads, cs.qkv_dim = spec.n_heads, spec.qkv_dim
        cs.n_layers = len(spec.hidden_structure)
        if cs.n_layers > _lib.MILE_MAX_LAYERS:
            raise ValueError(f'at most {_lib.MILE_MAX_LAYERS} layers')
        for i, w in enumerate(spec.hidden_structure):
            cs.widths[i] = w
        cs.activation = _lib.ACTIVATION_IDS[spec.activation]
        cs.task = _lib.TASK_IDS[spec.task]
        cs.prior = _lib.PRIOR_IDS[spec.prior]
        cs.prior_loc = spec.prior_loc
        cs.prior_scale = spec.prior_scale
        cs.use_bias = int(spec.use_bias)
        h = C.c_void_p()
        _lib.check(self.lib.mile_create(C.byref(cs), self.device.index or 0, C.byref(h)), self.lib)
        self._h = h
        self.d = int(self.lib.mile_param_count(h))
        assert self.d == spec.n_params
        self.dim = self.d                   # what init / step / tune / logpost_grad work on: d_s after set_partition
        self._frozen = None
        self._E_reserved = 0
        if isinstance(spec, PretrainedAttentionSpec):
            self.set_embedding(*(tables if tables is not None else spec.load_tables()))
        self.set_data(X, y)
        if grad_kernel != 'auto':
            self.set_grad_kernel(grad_kernel)

    def __del__(self):
        h = getattr(self, '_h', None)
        if h:
            self.lib.mile_destroy(h)
            self._h = None

    # ------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def set_data(self, X, y):
        X = _f32(X, self.device, name='X')
        if isinstance(self.spec, IMAGE_SPECS) and X.ndim == 4:    # [N, C, H, W] images -> rows of C*H*W
            if tuple(X.shape[1:]) != (self.spec.channels, self.spec.height, self.spec.width):
                raise ValueError(f'X must be [N, {self.spec.channels}, {self.spec.height}, {self.spec.width}], got {tuple(X.shape)}')
            X = X.reshape(X.shape[0], -1)
        if X.ndim != 2 or X.shape[1] != self.spec.in_features:
            raise ValueError(f'X must be [N, {self.spec.in_features}], got {tuple(X.shape)}')
        _check_tokens(self.spec, X)
        y = torch.as_tensor(y, device=self.device)
        if y.ndim == 2 and y.shape[1] == 1:
            y = y[:, 0]
        if y.shape != (X.shape[0],):
            raise ValueError(f'y must be [N], got {tuple(y.shape)}')
        if self.spec.task == 'regr':
            y = y.to(torch.float32).contiguous()
        else:
            y = y.to(torch.int32).contiguous()
            n_classes = self.spec.hidden_structure[-1]
            if int(y.min()) < 0 or int(y.max()) >= n_classes:
                raise ValueError('class labels out of range')
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_set_data(self._h, _ptr(X), _ptr(y), X.shape[0], self._stream()), self.lib)
            torch.cuda.current_stream(self.device).synchronize()   # X, y may be temporaries
        if int(X.shape[0]) != getattr(self, 'N', None):
            self._E_reserved = 0            # (same N: the library keeps its buffers and workspace)
        self.N = int(X.shape[0])

    def set_embedding(self, emb, pos):
        """The frozen tables of a PretrainedAttentionSpec: emb [V, C] and pos [>= T, C] (its first T rows are used), validated
        by spec.check_tables and copied into the library's own buffers."""
        emb, pos = self.spec.check_tables(emb, pos)
        emb = torch.from_numpy(emb).to(self.device)
        pos = torch.from_numpy(pos).to(self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_set_embedding(self._h, _ptr(emb), _ptr(pos), self._stream()), self.lib)
            torch.cuda.current_stream(self.device).synchronize()   # emb, pos are temporaries

    # ------------------------------------------------------------------ partition sampling
    def set_partition(self, frozen):
        """Partition mode (mile_set_partition): only the first and the last FCN layer are sampled; every other layer keeps,
        per chain, the values of ``frozen`` [E, d].  From here on ``init``, ``step``, ``tune`` and ``logpost_grad`` take and
        return compact [E, dim] tensors, dim = d_s; ``partition`` / ``merge`` convert.  ``pointwise_loglik``, ``predict``
        and ``warmstart_step`` stay full-layout.  A net with at most two layers has no frozen layer: dim stays d."""
        from mile_amd import partition as mpart
        frozen = _f32(frozen, self.device, name='frozen').clone()
        if frozen.ndim != 2 or frozen.shape[1] != self.d:
            raise ValueError(f'frozen must be [E, {self.d}], got {tuple(frozen.shape)}')
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_set_partition(self._h, _ptr(frozen), frozen.shape[0], self._stream()), self.lib)
            torch.cuda.current_stream(self.device).synchronize()
        self._E_reserved = 0
        self._frozen = frozen
        self.dim = int(self.lib.mile_partition_dim(self._h))
        segs = self.partition_segments
        if segs and segs != mpart.segments(self.spec):
            raise _lib.MileHipError(f'partition segments differ: library {segs}, host {mpart.segments(self.spec)}')
        self._part_idx = torch.as_tensor(mpart.sampled_index(self.spec), device=self.device)
        assert self.dim == self._part_idx.numel()

    @property
    def partitioned(self) -> bool:
        return self._frozen is not None

    @property
    def partition_segments(self) -> list:
        """[(begin, length)] of the sampled coordinates inside the full row (mile_partition_segments); [] outside partition
        mode (and for a net without a frozen layer)."""
        b, n = (C.c_int64 * 4)(), (C.c_int64 * 4)()
        k = self.lib.mile_partition_segments(self._h, b, n, 4)
        _lib.check(min(k, 0), self.lib)
        return [(int(b[i]), int(n[i])) for i in range(k)]

    def partition(self, full):
        """full [..., d] -> compact [..., dim]."""
        if not self.partitioned:
            raise ValueError('call set_partition first')
        full = _f32(full, self.device, name='full')
        if full.shape[-1] != self.d:
            raise ValueError(f'expected [..., {self.d}], got {tuple(full.shape)}')
        return full[..., self._part_idx].contiguous()

    def merge(self, compact):
        """compact [..., E, dim] -> full [..., E, d]: the frozen rows with the sampled coordinates replaced."""
        if not self.partitioned:
            raise ValueError('call set_partition first')
        from mile_amd import partition as mpart
        return mpart.merge(self.spec, _f32(compact, self.device, name='compact'), self._frozen)

    def set_row_window(self, begin: int = 0, count: int = 0):
        """Likelihood over rows [begin, begin + count) of the training set for the following logpost_grad calls
        (count = 0: all rows).  The minibatches of the warm-start stage."""
        _lib.check(self.lib.mile_set_row_window(self._h, int(begin), int(count)), self.lib)

    def reserve(self, E: int):
        # always asked: a SMALLER ensemble splits each particle's rows over more workgroups and may need more slab rows than
        # the larger one reserved (mile_reserve returns at once when the workspace already fits, and never shrinks it)
        _lib.check(self.lib.mile_reserve(self._h, int(E)), self.lib)
        self._E_reserved = max(self._E_reserved, int(E))

    @property
    def slab_bytes(self) -> int:
        """Bytes of the gradient slabs the library holds now (mile_slab_bytes)."""
        return int(self.lib.mile_slab_bytes(self._h))

    def set_grad_kernel(self, name: str):
        _lib.check(self.lib.mile_set_grad_kernel(self._h, _lib.GRAD_KERNEL_IDS[name]), self.lib)

    @property
    def grad_kernel(self) -> str:
        k = self.lib.mile_get_grad_kernel(self._h)
        return {v: n for n, v in _lib.GRAD_KERNEL_IDS.items()}[k]

    def grad_launch_info(self, E: int) -> dict:
        gx, gy, blk, lds = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        name = C.create_string_buffer(64)
        _lib.check(self.lib.mile_grad_launch_info(self._h, E, C.byref(gx), C.byref(gy), C.byref(blk),
                                                  C.byref(lds), name, 64), self.lib)
        return {'kernel': name.value.decode(), 'grid': (gx.value, gy.value), 'block': blk.value,
                'lds_bytes': lds.value}

    def grad_timing_begin(self):
        _lib.check(self.lib.mile_grad_timing_begin(self._h), self.lib)

    def grad_timing_end(self):
        ms, n = C.c_float(), C.c_int32()
        _lib.check(self.lib.mile_grad_timing_end(self._h, C.byref(ms), C.byref(n)), self.lib)
        return float(ms.value), int(n.value)

    # ------------------------------------------------------------------
    def logpost_grad(self, theta):
        """jax.value_and_grad(logdensity_fn) for an ensemble: theta [E, d] -> (logp [E], grad [E, d])."""
        theta = _f32(theta, self.device, name='theta')
        if theta.ndim != 2 or theta.shape[1] != self.dim:
            raise ValueError(f'theta must be [E, {self.dim}], got {tuple(theta.shape)}')
        E = theta.shape[0]
        self.reserve(E)
        logp = torch.empty(E, dtype=torch.float32, device=self.device)
        grad = torch.empty_like(theta)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_logpost_grad(self._h, _ptr(theta), E, _ptr(logp), _ptr(grad),
                                                  self._stream()), self.lib)
        return logp, grad

    def warmstart_step(self, theta: torch.Tensor, optim: dict, active: torch.Tensor | None = None,
                       want_nll: bool = False) -> torch.Tensor | None:
        """One optimizer step of all members on the current row window (mile_warmstart_step): likelihood gradient from the
        grad kernel + ONE fused optimizer launch.  ``theta`` [E, d] and the moments ``optim['m']``, ``optim['v']`` are
        updated IN PLACE; ``optim`` also carries name, learning_rate, b1, b2, eps, weight_decay and the step count ``t``
        (incremented here).  ``active`` [E] uint8 / bool: 0 freezes a member (early stopping)."""
        if theta.dtype != torch.float32 or not theta.is_contiguous() or theta.device != self.device or theta.shape[1] != self.d:
            raise ValueError(f'theta must be a contiguous fp32 [E, {self.d}] tensor on the engine device')
        E = theta.shape[0]
        self.reserve(E)
        a = _lib.OptimArgsC()
        a.kind = _lib.OPTIMIZER_IDS[optim['name']]
        a.learning_rate, a.b1, a.b2 = optim['learning_rate'], optim['b1'], optim['b2']
        a.eps, a.weight_decay = optim['eps'], optim['weight_decay']
        optim['t'] += 1
        a.t = optim['t']
        if a.kind != 0:
            for k in ('m', 'v'):
                t = optim[k]
                if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != theta.shape or t.device != self.device:
                    raise ValueError('optimizer moments must match theta')
            a.m, a.v = optim['m'].data_ptr(), optim['v'].data_ptr()
        act = None
        if active is not None:
            act = active.to(device=self.device, dtype=torch.uint8).contiguous()
            a.active = act.data_ptr()
        nll = torch.empty(E, dtype=torch.float32, device=self.device) if want_nll else None
        a.out_nll = nll.data_ptr() if nll is not None else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_warmstart_step(self._h, _ptr(theta), E, C.byref(a), self._stream()), self.lib)
        return nll

    def _state_c(self, st: IntegratorState):
        sc = _lib.StateC()
        sc.n_particles = st.position.shape[0]
        sc.position = st.position.data_ptr()
        sc.momentum = st.momentum.data_ptr()
        sc.logdensity = st.logdensity.data_ptr()
        sc.logdensity_grad = st.logdensity_grad.data_ptr()
        return sc

    def _ids(self, particle_ids, E):
        if particle_ids is None:
            return None
        ids = torch.as_tensor(particle_ids, device=self.device).to(torch.int32).contiguous()
        if ids.shape != (E,):
            raise ValueError(f'particle_ids must be [{E}]')
        return ids

    def _mclmc_args(self, a, state, tuner, step_size, L, n_steps, noise, seed, step_offset, particle_ids, refresh,
                    sqrt_diag_cov):
        """Checks the state and fills what StepArgsC and TuneArgsC share.  ``tuner``: mile_tune's tensors (its step size
        among them), or None for mile_step and its ``step_size``.  Returns the tensors ``a`` points into: they must outlive
        the call."""
        E, dev = state.position.shape[0], self.device
        what, tensors = ('state', tuple(state)) if tuner is None else ('state / tuner', tuple(state) + tuple(tuner.values()))
        for t in tensors:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise ValueError(f'{what} tensors must be contiguous fp32 on the engine device')
        if tuner is not None and tuner['stream_average'].shape != (E, 2, self.dim):
            raise ValueError('stream_average must be [E, 2, d]')
        self.reserve(E)
        if tuner is not None:
            eps = tuner['step_size']
        elif torch.as_tensor(step_size).ndim == 0:
            eps = _f32(step_size, dev).expand(E).contiguous()
        else:
            eps = _f32(step_size, dev, (E,), 'step_size')
        Lt = _f32(L, dev).expand(E).contiguous() if torch.as_tensor(L).ndim == 0 else _f32(L, dev, (E,), 'L')
        z = _f32(noise, dev, (n_steps, 2, E, self.dim), 'noise') if noise is not None else None
        sdc = _f32(sqrt_diag_cov, dev, (E, self.dim), 'sqrt_diag_cov') if sqrt_diag_cov is not None else None
        ids = self._ids(particle_ids, E)
        a.step_size = eps.data_ptr()
        a.L = Lt.data_ptr()
        a.sqrt_diag_cov = sdc.data_ptr() if sdc is not None else None
        a.noise = z.data_ptr() if z is not None else None
        a.seed = seed
        a.particle_ids = ids.data_ptr() if ids is not None else None
        a.step_offset = step_offset
        a.n_steps = n_steps
        a.refresh = _lib.REFRESH_IDS[refresh]
        return eps, Lt, z, sdc, ids

    def init(self, position, noise=None, seed: int = 0, particle_ids=None) -> IntegratorState:
        """blackjax.mcmc.mclmc.init for an ensemble.  ``noise`` [E, d] (explicit N(0,1) draws)
        or the counter RNG keyed by (seed, particle id)."""
        position = _f32(position, self.device, name='position').clone()
        if position.ndim != 2 or position.shape[1] != self.dim:
            raise ValueError(f'position must be [E, {self.dim}], got {tuple(position.shape)}')
        if self.dim < 2:
            raise ValueError('The target distribution must have more than 1 dimension for MCLMC.')
        E = position.shape[0]
        self.reserve(E)
        st = IntegratorState(position, torch.empty_like(position),
                             torch.empty(E, dtype=torch.float32, device=self.device),
                             torch.empty_like(position))
        z = _f32(noise, self.device, (E, self.dim), 'noise') if noise is not None else None
        ids = self._ids(particle_ids, E)
        sc = self._state_c(st)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_init(self._h, C.byref(sc), _ptr(z), C.c_uint64(seed), _ptr(ids),
                                          self._stream()), self.lib)
        return st

    def step(self, state: IntegratorState, step_size, L, n_steps: int = 1, *, noise=None, seed: int = 0,
             step_offset: int = 0, n_thinning: int = 0, particle_ids=None, refresh: str = 'O-step-O',
             sqrt_diag_cov=None, want_info: bool = True, inplace: bool = False):
        """n_steps kernel steps.  Returns (state, MCLMCInfo | None, samples [n_kept, E, d] | None).

        Pure by default (the input state is cloned, as blackjax's step is functional);
        ``inplace=True`` advances the given tensors.
        """
        E = state.position.shape[0]
        dev = self.device
        if not inplace:
            state = IntegratorState(*(t.clone() for t in state))
        a = _lib.StepArgsC()
        keep = self._mclmc_args(a, state, None, step_size, L, n_steps, noise, seed, step_offset, particle_ids, refresh,
                                sqrt_diag_cov)
        n_kept = 0
        if n_thinning > 0:
            n_kept = sum(1 for i in range(n_steps) if (step_offset + i) % n_thinning == 0)
        samples = torch.empty((n_kept, E, self.dim), dtype=torch.float32, device=dev) if n_kept else None
        info = torch.empty((n_steps, E, 3), dtype=torch.float32, device=dev) if want_info else None
        a.n_thinning = n_thinning
        a.out_samples = samples.data_ptr() if samples is not None else None
        a.out_info = info.data_ptr() if info is not None else None
        sc = self._state_c(state)
        with torch.cuda.device(dev):
            _lib.check(self.lib.mile_step(self._h, C.byref(sc), C.byref(a), self._stream()), self.lib)
        inf = MCLMCInfo(info[..., 0], info[..., 1], info[..., 2]) if info is not None else None
        return state, inf, samples

    def tune(self, state: IntegratorState, tuner: dict, L, n_steps: int, *, schedule_step0: int, n_mask_steps: int,
             schedule_total: int, desired_energy_var_start: float, desired_energy_var_end: float,
             trust_in_estimate: float, decay_rate: float, noise=None, seed: int = 0, step_offset: int = 0,
             particle_ids=None, refresh: str = 'O-step-O', sqrt_diag_cov=None, want_info: bool = False):
        """n_steps warm-up steps with on-device step-size adaptation (mile_tune).  ``state`` and the
        ``tuner`` tensors (step_size, step_size_max, time, x_average, stream_weight [E];
        stream_average [E, 2, d]) are advanced IN PLACE.  Returns MCLMCInfo or None."""
        E, dev = state.position.shape[0], self.device
        a = _lib.TuneArgsC()
        keep = self._mclmc_args(a, state, tuner, None, L, n_steps, noise, seed, step_offset, particle_ids, refresh,
                                sqrt_diag_cov)
        info = torch.empty((n_steps, E, 3), dtype=torch.float32, device=dev) if want_info else None
        a.step_size_max = tuner['step_size_max'].data_ptr()
        a.time = tuner['time'].data_ptr()
        a.x_average = tuner['x_average'].data_ptr()
        a.stream_weight = tuner['stream_weight'].data_ptr()
        a.stream_average = tuner['stream_average'].data_ptr()
        a.schedule_step0 = schedule_step0
        a.n_mask_steps = n_mask_steps
        a.schedule_total = schedule_total
        a.desired_energy_var_start = desired_energy_var_start
        a.desired_energy_var_end = desired_energy_var_end
        a.trust_in_estimate = trust_in_estimate
        a.decay_rate = decay_rate
        a.out_info = info.data_ptr() if info is not None else None
        sc = self._state_c(state)
        with torch.cuda.device(dev):
            _lib.check(self.lib.mile_tune(self._h, C.byref(sc), C.byref(a), self._stream()), self.lib)
        return MCLMCInfo(info[..., 0], info[..., 1], info[..., 2]) if info is not None else None

    # ------------------------------------------------------------------ NUTS
    def nuts_reserve(self, E: int, max_num_doublings: int):
        self.reserve(E)
        _lib.check(self.lib.mile_nuts_reserve(self._h, int(E), int(max_num_doublings)), self.lib)

    def nuts_init(self, position) -> HMCState:
        """blackjax.nuts init: the log density and its gradient at ``position`` [E, d]."""
        position = _f32(position, self.device, name='position').clone()
        if position.ndim != 2 or position.shape[1] != self.d:
            raise ValueError(f'position must be [E, {self.d}], got {tuple(position.shape)}')
        logp, grad = self.logpost_grad(position)
        return HMCState(position, logp, grad)

    def _nuts_args(self, state: HMCState, n_steps, max_num_doublings, divergence_threshold, noise, uniforms, seed,
                   step_offset, n_thinning, particle_ids, want_info, stats):
        E, dev = state.position.shape[0], self.device
        for t in state:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise ValueError('state tensors must be contiguous fp32 on the engine device')
        M = int(max_num_doublings)
        self.nuts_reserve(E, M)
        keep = {}
        z = _f32(noise, dev, (n_steps, E, self.d), 'noise') if noise is not None else None
        u = _f32(uniforms, dev, (n_steps, E, 2 * M + 2 ** M), 'uniforms') if uniforms is not None else None
        ids = self._ids(particle_ids, E)
        n_kept = sum(1 for i in range(n_steps) if (step_offset + i) % n_thinning == 0) if n_thinning > 0 else 0
        samples = torch.empty((n_kept, E, self.d), dtype=torch.float32, device=dev) if n_kept else None
        info = torch.empty((n_steps, E, 6), dtype=torch.float32, device=dev) if want_info else None
        a = _lib.NutsArgsC()
        a.max_num_doublings = M
        a.divergence_threshold = float(divergence_threshold)
        a.momentum_noise = z.data_ptr() if z is not None else None
        a.uniforms = u.data_ptr() if u is not None else None
        a.seed = seed
        a.particle_ids = ids.data_ptr() if ids is not None else None
        a.step_offset = step_offset
        a.n_steps = n_steps
        a.n_thinning = n_thinning
        a.out_samples = samples.data_ptr() if samples is not None else None
        a.out_info = info.data_ptr() if info is not None else None
        if stats is not None:
            a.out_stats = stats
        keep.update(z=z, u=u, ids=ids)
        return a, keep, samples, info

    @staticmethod
    def _nuts_info(info):
        return NUTSInfo(*(info[..., k] for k in range(6))) if info is not None else None

    def nuts_step(self, state: HMCState, step_size, inverse_mass_matrix, n_steps: int = 1, *, max_num_doublings: int = 10,
                  divergence_threshold: float = 1000.0, noise=None, uniforms=None, seed: int = 0, step_offset: int = 0,
                  n_thinning: int = 0, particle_ids=None, want_info: bool = True, inplace: bool = False, stats=None):
        """n_steps NUTS steps of all chains in lockstep (mile_nuts_step).  ``noise`` [n_steps, E, d] and ``uniforms``
        [n_steps, E, 2 M + 2^M]: explicit draws (slot layout of include/mile_hip.h), else the counter RNG.
        Returns (state, NUTSInfo | None, samples [n_kept, E, d] | None).  ``stats``: a ctypes int64[2] that receives the
        leapfrog rounds launched and host syncs (added to)."""
        E, dev = state.position.shape[0], self.device
        if not inplace:
            state = HMCState(*(t.clone() for t in state))
        eps = _f32(step_size, dev).expand(E).contiguous() if torch.as_tensor(step_size).ndim == 0 \
            else _f32(step_size, dev, (E,), 'step_size')
        imm = torch.as_tensor(inverse_mass_matrix)
        imm = _f32(imm, dev).expand(E, self.d).contiguous() if imm.ndim < 2 else _f32(imm, dev, (E, self.d), 'inverse_mass_matrix')
        a, keep, samples, info = self._nuts_args(state, n_steps, max_num_doublings, divergence_threshold, noise, uniforms,
                                                 seed, step_offset, n_thinning, particle_ids, want_info, stats)
        a.step_size = eps.data_ptr()
        a.inverse_mass_matrix = imm.data_ptr()
        sc = _lib.StateC()
        sc.n_particles = E
        sc.position, sc.logdensity, sc.logdensity_grad = (state.position.data_ptr(), state.logdensity.data_ptr(),
                                                          state.logdensity_grad.data_ptr())
        with torch.cuda.device(dev):
            _lib.check(self.lib.mile_nuts_step(self._h, C.byref(sc), C.byref(a), self._stream()), self.lib)
        return state, self._nuts_info(info), samples

    def nuts_adaptation_init(self, E: int, initial_step_size: float = 1.0) -> dict:
        """window_adaptation.base init per chain: the caller-owned state mile_nuts_warmup updates in place."""
        dev = self.device
        ad = {'step_size': torch.full((E,), float(initial_step_size), dtype=torch.float32, device=dev),
              'inverse_mass_matrix': torch.ones((E, self.d), dtype=torch.float32, device=dev),
              'da': torch.tensor([math.log(initial_step_size), 0.0, 1.0, 0.0, math.log(10 * initial_step_size)],
                                 dtype=torch.float32, device=dev).repeat(E, 1).contiguous(),
              'welford': torch.zeros((E, 2, self.d), dtype=torch.float32, device=dev),
              'welford_count': torch.zeros(E, dtype=torch.float32, device=dev)}
        return ad

    def nuts_warmup(self, state: HMCState, adaptation: dict, schedule, *, max_num_doublings: int = 10,
                    divergence_threshold: float = 1000.0, target_acceptance_rate: float = 0.8, noise=None, uniforms=None,
                    seed: int = 0, step_offset: int = 0, n_thinning: int = 0, particle_ids=None, want_info: bool = False,
                    stats=None):
        """len(schedule) NUTS steps with the window adaptation on the device (mile_nuts_warmup).  ``state`` and the
        ``adaptation`` tensors advance IN PLACE; ``schedule`` [n_steps, 2] (stage, is_middle_window_end) from
        warmup.build_schedule.  Returns (NUTSInfo | None, kept positions | None)."""
        sch = (C.c_int32 * (2 * len(schedule)))(*[int(v) for row in schedule for v in row])
        n_steps = len(schedule)
        E = state.position.shape[0]
        for k, t in adaptation.items():
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device or t.shape[0] != E:
                raise ValueError(f'adaptation[{k!r}] must be a contiguous fp32 tensor of {E} rows on the engine device')
        a, keep, samples, info = self._nuts_args(state, n_steps, max_num_doublings, divergence_threshold, noise, uniforms,
                                                 seed, step_offset, n_thinning, particle_ids, want_info, stats)
        w = _lib.NutsAdaptArgsC()
        w.step_size = adaptation['step_size'].data_ptr()
        w.inverse_mass_matrix = adaptation['inverse_mass_matrix'].data_ptr()
        w.da = adaptation['da'].data_ptr()
        w.welford = adaptation['welford'].data_ptr()
        w.welford_count = adaptation['welford_count'].data_ptr()
        w.schedule = C.cast(sch, C.POINTER(C.c_int32))
        w.target_acceptance_rate = float(target_acceptance_rate)
        sc = _lib.StateC()
        sc.n_particles = E
        sc.position, sc.logdensity, sc.logdensity_grad = (state.position.data_ptr(), state.logdensity.data_ptr(),
                                                          state.logdensity_grad.data_ptr())
        if n_steps:
            with torch.cuda.device(self.device):
                _lib.check(self.lib.mile_nuts_warmup(self._h, C.byref(sc), C.byref(a), C.byref(w), self._stream()), self.lib)
        return self._nuts_info(info), samples

    def _eval_inputs(self, theta, X, y=None, *, name_x: str = 'X'):
        """The inputs every evaluation method shares, checked and on the device: (leading shape of theta, theta [*, d] fp32,
        X [N, F] fp32 with images flattened, y [N] fp32 / int32 by task or None)."""
        theta = _f32(theta, self.device, name='theta')
        th = theta.reshape(-1, self.d).contiguous()
        X = _f32(X, self.device, name=name_x)
        if isinstance(self.spec, IMAGE_SPECS) and X.ndim == 4:
            X = X.reshape(X.shape[0], -1).contiguous()
        ok = X.ndim == 2 and X.shape[1] == self.spec.in_features
        if y is None:
            if not ok:
                raise ValueError(f'{name_x} must be [N, F]')
        else:
            y = torch.as_tensor(y, device=self.device)
            y = (y.to(torch.float32) if self.spec.task == 'regr' else y.to(torch.int32)).contiguous()
            if not ok or y.shape != (X.shape[0],):
                raise ValueError(f'{name_x} must be [N, F] and y [N]')
        _check_tokens(self.spec, X)
        if y is not None and self.spec.task != 'regr' and y.numel():       # the kernels index the logits with the raw label
            if int(y.min()) < 0 or int(y.max()) >= self.spec.hidden_structure[-1]:
                raise ValueError('class labels out of range')
        return theta.shape[:-1], th, X, y

    def pointwise_loglik(self, theta, X, y) -> torch.Tensor:
        """log p(y_n | x_n, theta_s) for every sample and test row: theta [..., d] -> [..., N]
        (pointwise_lppd's input, src/inference/metrics.py:247-294), computed by the HIP forward kernels."""
        lead, th, X, y = self._eval_inputs(theta, X, y)
        out = torch.empty((th.shape[0], X.shape[0]), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_pointwise_loglik(self._h, _ptr(th), th.shape[0], _ptr(X), _ptr(y), X.shape[0],
                                                      _ptr(out), self._stream()), self.lib)
        return out.reshape(*lead, X.shape[0])

    def predict(self, theta, X) -> torch.Tensor:
        """Raw network outputs for every sample and test row: theta [..., d] -> [..., N, O], O the width of the last layer
        (``module.apply`` in predict_from_samples, src/inference/evaluation.py:16-43): (mu, log sigma) unclipped or the
        logits, NaN / inf untouched.  Computed by the HIP forward kernels of pointwise_loglik (mile_predict)."""
        lead, th, X, _ = self._eval_inputs(theta, X)
        O = self.spec.hidden_structure[-1]
        out = torch.empty((th.shape[0], X.shape[0], O), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_predict(self._h, _ptr(th), th.shape[0], _ptr(X), X.shape[0], _ptr(out),
                                             self._stream()), self.lib)
        return out.reshape(*lead, X.shape[0], O)

    def predict_moments(self, theta, X, *, max_draws_per_pass: int = 0, return_dropped: bool = False):
        """Posterior-predictive moments of all draws theta [..., d] on X [N, F], reduced on the device (mile_predict_moments):
        [N, 3] = (mean, epistemic variance, aleatoric variance) for regression, [N, K + 2] = (mean class probabilities,
        predictive entropy, mutual information) for classification -- ``metrics.predictive_moments`` of ``predict``'s
        outputs, without ever holding them.  ``max_draws_per_pass`` bounds the draws forwarded at a time (0: the library's
        choice).  A draw with a non-finite output on a row is left out of that row; ``return_dropped`` also returns how many
        were, int32 [N]."""
        _, th, X, _ = self._eval_inputs(theta, X)
        W = int(self.lib.mile_predict_moments_width(self._h))
        out = torch.empty((X.shape[0], W), dtype=torch.float32, device=self.device)
        dropped = torch.empty(X.shape[0], dtype=torch.int32, device=self.device) if return_dropped else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_predict_moments(self._h, _ptr(th), th.shape[0], _ptr(X), X.shape[0], _ptr(out),
                                                     _ptr(dropped), int(max_draws_per_pass), self._stream()), self.lib)
        return (out, dropped) if return_dropped else out

    @staticmethod
    def _quantile_levels(levels):
        lv = [float(v) for v in torch.as_tensor(levels, dtype=torch.float64).reshape(-1)]
        if not 1 <= len(lv) <= 32:
            raise ValueError('levels: between 1 and 32 of them')
        if not all(0.0 < v < 1.0 for v in lv):
            raise ValueError('levels must lie strictly inside (0, 1)')
        if not all(a < b for a, b in zip(lv, lv[1:])):
            raise ValueError('levels must be strictly increasing')
        return (C.c_double * len(lv))(*lv), len(lv)

    def _quantile_outputs(self, N, Q, y, return_dropped):
        if y is not None:
            y = torch.as_tensor(y, device=self.device).to(torch.float32).reshape(-1).contiguous()
            if y.shape != (N,):
                raise ValueError('y must be [N]')
        quant = torch.empty((N, Q), dtype=torch.float32, device=self.device)
        pit = torch.empty(N, dtype=torch.float32, device=self.device) if y is not None else None
        dropped = torch.empty(N, dtype=torch.int32, device=self.device) if return_dropped else None
        return y, quant, pit, dropped

    @staticmethod
    def _quantile_result(quant, pit, dropped):
        res = (quant,) + ((pit,) if pit is not None else ()) + ((dropped,) if dropped is not None else ())
        return res if len(res) > 1 else quant

    def mixture_quantiles(self, raw, levels, y=None, return_dropped: bool = False):
        """Exact quantiles of the equal-weight mixture of Normals that raw outputs [..., N, 2] (mu, log sigma; every leading
        axis is a draw axis) describe on each row, at ``levels`` (strictly increasing, strictly inside (0, 1), at most 32),
        by the library's bracketed solver (mile_mixture_quantiles): [N, Q] fp32, non-decreasing along Q.  With ``y`` [N] also
        the probability integral transform F_n(y_n), [N] fp32; ``return_dropped`` appends the draws left out of each row for
        a non-finite output, int32 [N].  The outputs may come from anywhere -- ``predict``, or a deep ensemble's members."""
        lv, Q = self._quantile_levels(levels)
        raw = _f32(raw, self.device, name='raw')
        if raw.ndim < 2 or raw.shape[-1] != 2:
            raise ValueError('raw must be [..., N, 2]')
        N = int(raw.shape[-2])
        r = raw.reshape(-1, N, 2).contiguous()
        y, quant, pit, dropped = self._quantile_outputs(N, Q, y, return_dropped)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_mixture_quantiles(_ptr(r), r.shape[0], N, lv, Q, _ptr(y), _ptr(quant), _ptr(pit),
                                                       _ptr(dropped), self._stream()), self.lib)
        return self._quantile_result(quant, pit, dropped)

    def predict_quantiles_workspace(self, S: int, N: int) -> int:
        """Bytes of the workspace ``predict_quantiles`` keeps in the handle for S draws on N rows with the library's own
        tile (mile_predict_quantiles_workspace)."""
        return int(self.lib.mile_predict_quantiles_workspace(self._h, int(S), int(N)))

    def predict_quantiles(self, theta, X, levels, y=None, *, max_draws_per_pass: int = 0, max_rows_per_tile: int = 0,
                          return_dropped: bool = False):
        """``mixture_quantiles`` of ``predict``'s outputs for draws theta [..., d] on X [N, F] without ever holding them
        (mile_predict_quantiles): the rows go in tiles of at most ``max_rows_per_tile`` (0: the library's choice), the forward
        inside a tile in passes of at most ``max_draws_per_pass`` draws (0: all).  Returns ``quant`` [N, Q] fp32, and ``pit``
        [N] when ``y`` is given; ``return_dropped`` appends the draws left out of each row.  The result does not depend on the
        two sizes, bit for bit.  Regression only."""
        if self.spec.task != 'regr':
            raise ValueError('predict_quantiles: a regression model is needed')
        lv, Q = self._quantile_levels(levels)
        _, th, X, _ = self._eval_inputs(theta, X)
        N = int(X.shape[0])
        y, quant, pit, dropped = self._quantile_outputs(N, Q, y, return_dropped)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_predict_quantiles(self._h, _ptr(th), th.shape[0], _ptr(X), N, lv, Q, _ptr(y), _ptr(quant),
                                                       _ptr(pit), _ptr(dropped), int(max_draws_per_pass), int(max_rows_per_tile),
                                                       self._stream()), self.lib)
        return self._quantile_result(quant, pit, dropped)

    @staticmethod
    def _chain_weights(weights, n_chains):
        from .metrics import chain_weights
        return (C.c_double * n_chains)(*[float(v) for v in chain_weights(weights, n_chains)])

    def mixture_quantiles_weighted(self, raw, weights, levels, y=None, return_dropped: bool = False):
        """``mixture_quantiles`` for the chain-weighted mixture (mile_mixture_quantiles_weighted): raw [C, S, N, 2], chain c
        with weight ``weights[c]`` (>= 0, summing to 1; stacking weights), F_n(t) = sum_c (w_c / K_c) sum_kept Phi(.).  A chain
        with weight 0 enters no sum; a row on which a weighted chain has no finite draw is NaN.  ``return_dropped`` appends the
        draws left out per chain and row, int32 [C, N]."""
        lv, Q = self._quantile_levels(levels)
        raw = _f32(raw, self.device, name='raw')
        if raw.ndim != 4 or raw.shape[-1] != 2:
            raise ValueError('raw must be [C, S, N, 2]')
        n_chains, S, N = (int(v) for v in raw.shape[:3])
        w = self._chain_weights(weights, n_chains)
        r = raw.contiguous()
        y, quant, pit, _ = self._quantile_outputs(N, Q, y, False)
        dropped = torch.empty((n_chains, N), dtype=torch.int32, device=self.device) if return_dropped else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_mixture_quantiles_weighted(_ptr(r), n_chains, S, N, w, lv, Q, _ptr(y), _ptr(quant), _ptr(pit),
                                                                _ptr(dropped), self._stream()), self.lib)
        return self._quantile_result(quant, pit, dropped)

    def predict_quantiles_weighted_workspace(self, C: int, S: int, N: int) -> int:
        """Bytes of the workspace ``predict_quantiles_weighted`` keeps in the handle for C chains of S draws on N rows with the
        library's own tile (mile_predict_quantiles_weighted_workspace)."""
        return int(self.lib.mile_predict_quantiles_weighted_workspace(self._h, int(C), int(S), int(N)))

    def predict_quantiles_weighted(self, theta, X, weights, levels, y=None, *, max_draws_per_pass: int = 0,
                                   max_rows_per_tile: int = 0, return_dropped: bool = False):
        """``mixture_quantiles_weighted`` of ``predict``'s outputs for draws theta [C, S, d] on X [N, F] without ever holding
        them (mile_predict_quantiles_weighted), with ``predict_quantiles``' tiles and passes; the result does not depend on the
        two sizes, bit for bit.  Regression only."""
        if self.spec.task != 'regr':
            raise ValueError('predict_quantiles_weighted: a regression model is needed')
        lv, Q = self._quantile_levels(levels)
        lead, th, X, _ = self._eval_inputs(theta, X)
        if len(lead) != 2:
            raise ValueError('theta must be [C, S, d]')
        n_chains, S = int(lead[0]), int(lead[1])
        w = self._chain_weights(weights, n_chains)
        N = int(X.shape[0])
        y, quant, pit, _ = self._quantile_outputs(N, Q, y, False)
        dropped = torch.empty((n_chains, N), dtype=torch.int32, device=self.device) if return_dropped else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_predict_quantiles_weighted(self._h, _ptr(th), n_chains, S, _ptr(X), N, w, lv, Q, _ptr(y),
                                                                _ptr(quant), _ptr(pit), _ptr(dropped), int(max_draws_per_pass),
                                                                int(max_rows_per_tile), self._stream()), self.lib)
        return self._quantile_result(quant, pit, dropped)

    def predict_moments_by_chain(self, theta, X, *, max_draws_per_pass: int = 0):
        """``predict_moments`` of each chain's draws: theta [C, S, d] -> (moments [C, N, W] fp32, kept [C, N] int32, the
        chain's draws with finite outputs on the row) -- what ``metrics.weighted_moments`` and ``weighted_class_probs``
        combine.  The same forwards in all as one ``predict_moments`` of every draw."""
        theta = _f32(theta, self.device, name='theta')
        if theta.ndim != 3:
            raise ValueError('theta must be [C, S, d]')
        res = [self.predict_moments(theta[c], X, max_draws_per_pass=max_draws_per_pass, return_dropped=True)
               for c in range(theta.shape[0])]
        return torch.stack([m for m, _ in res]), torch.stack([int(theta.shape[1]) - d for _, d in res])

    def predict_sensitivities_workspace(self, C: int, S: int, N: int) -> int:
        """Bytes of the handle's workspace ``predict_sensitivities`` needs for C chains of S draws on N rows with the library's
        tile and pass, -1 where the call would be refused (mile_predict_sensitivities_workspace)."""
        return int(self.lib.mile_predict_sensitivities_workspace(self._h, int(C), int(S), int(N)))

    def predict_sensitivities(self, samples, X, *, max_draws_per_pass: int = 0, max_rows_per_tile: int = 0) -> dict:
        """Input sensitivities of the ensemble's predictions, reduced on the device (mile_predict_sensitivities; FCN only):
        per draw and row the Jacobian J[p][f] of the head outputs -- mu and log sigma for regression, the class probabilities
        for classification -- with respect to the row's inputs, by one forward and P backward sweeps in a HIP kernel.
        ``samples`` [C, S, d] or [S, d] (one chain), ``X`` [N, F].  Returns tensors on the device: ``mean``, ``sd``, ``pos``
        fp32 [N, P, F] over the kept draws of all chains (sd with ddof 1, the epistemic spread of the effect; pos the share of
        draws with J > 0), ``dropped`` int32 [N], and per chain over its kept (draw, row) pairs ``chain_ape`` (the average partial
        effect), ``chain_abs`` (the importance) fp64 [C, P, F] and ``chain_kept`` int64 [C].  A (draw, row) pair with a non-finite
        raw output or Jacobian entry is left out of that row.  Rows go in tiles of at most ``max_rows_per_tile``, draws in passes
        of at most ``max_draws_per_pass`` (0: the library's choice); ``metrics.sensitivities_dense`` is the same in torch."""
        samples = _f32(samples, self.device, name='samples')
        if samples.ndim == 2:
            samples = samples[None]
        if samples.ndim != 3 or samples.shape[2] != self.d:
            raise ValueError(f'samples must be [C, S, {self.d}] or [S, {self.d}]')
        (C_, S_), theta, X, _ = self._eval_inputs(samples, X)
        N, F, P = int(X.shape[0]), int(X.shape[1]), int(self.spec.hidden_structure[-1])
        new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=self.device)
        out = {'mean': new(torch.float32, N, P, F), 'sd': new(torch.float32, N, P, F), 'pos': new(torch.float32, N, P, F),
               'dropped': new(torch.int32, N), 'chain_ape': new(torch.float64, C_, P, F), 'chain_abs': new(torch.float64, C_, P, F),
               'chain_kept': new(torch.int64, C_)}
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_predict_sensitivities(self._h, _ptr(theta), C_, S_, _ptr(X), N, int(max_draws_per_pass),
                                                           int(max_rows_per_tile), *[_ptr(out[k]) for k in
                                                                                     ('mean', 'sd', 'pos', 'dropped', 'chain_ape', 'chain_abs', 'chain_kept')],
                                                           self._stream()), self.lib)
        return out

    PD_OUTPUTS = ('ice_mean', 'ice_sd', 'dropped', 'curves', 'pd_mean', 'pd_sd', 'chain_pd', 'chain_draws')

    def predict_partial_dependence_workspace(self, C: int, S: int, N: int, Fs: int, G: int) -> int:
        """Bytes of the handle's workspace ``predict_partial_dependence`` needs for C chains of S draws on N rows, Fs features
        and G grid points with the library's tile and pass, -1 where the call would be refused
        (mile_predict_partial_dependence_workspace)."""
        return int(self.lib.mile_predict_partial_dependence_workspace(self._h, int(C), int(S), int(N), int(Fs), int(G)))

    def predict_partial_dependence(self, samples, x, features, grid, max_draws_per_pass: int = 0, max_rows_per_tile: int = 0,
                                   want=PD_OUTPUTS) -> dict:
        """Partial dependence and ICE curves of the ensemble's predictions, reduced on the device
        (mile_predict_partial_dependence; FCN only): per draw, row, feature ``features[i]`` and grid value ``grid[i][g]`` the head
        outputs -- mu and log sigma for regression, the class probabilities for classification -- of the row with that input
        replaced by the grid value, in a HIP kernel that computes the first layer once per (draw, row).  ``samples`` [C, S, d]
        or [S, d] (one chain), ``x`` [N, F], ``features`` [Fs] distinct indices, ``grid`` [Fs, G].  Returns the tensors named in
        ``want``, on the device: ``ice_mean``, ``ice_sd`` fp32 [N, Fs, G, P] over the kept draws of all chains (sd with ddof 1),
        ``dropped`` int32 [N, Fs]; ``curves`` fp32 [C * S, Fs, G, P], each draw's mean over its kept rows; ``pd_mean``, ``pd_sd``
        fp64 [Fs, G, P] over the draws that have a curve (the posterior band); ``chain_pd`` fp64 [C, Fs, G, P] and
        ``chain_draws`` int64 [C, Fs].  A (draw, row, feature) with a non-finite value anywhere on the feature's grid is left
        out.  Rows go in tiles of at most ``max_rows_per_tile``, draws in passes of at most ``max_draws_per_pass`` (0: the
        library's choice); ``metrics.partial_dependence_dense`` is the same in torch."""
        samples = _f32(samples, self.device, name='samples')
        if samples.ndim == 2:
            samples = samples[None]
        if samples.ndim != 3 or samples.shape[2] != self.d:
            raise ValueError(f'samples must be [C, S, {self.d}] or [S, {self.d}]')
        (C_, S_), theta, x, _ = self._eval_inputs(samples, x, name_x='x')
        feats = [int(f) for f in features]
        grid = _f32(grid, self.device, name='grid')
        if grid.ndim != 2 or grid.shape[0] != len(feats) or grid.shape[1] < 1:
            raise ValueError('grid must be [Fs, G] with one row per feature')
        grid = grid.contiguous()
        unknown = [k for k in want if k not in self.PD_OUTPUTS]
        if unknown or not want:
            raise ValueError(f'want: some of {self.PD_OUTPUTS}')
        N, Fs, G, P = int(x.shape[0]), len(feats), int(grid.shape[1]), int(self.spec.hidden_structure[-1])
        new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=self.device)
        shapes = {'ice_mean': (torch.float32, N, Fs, G, P), 'ice_sd': (torch.float32, N, Fs, G, P), 'dropped': (torch.int32, N, Fs),
                  'curves': (torch.float32, C_ * S_, Fs, G, P), 'pd_mean': (torch.float64, Fs, G, P), 'pd_sd': (torch.float64, Fs, G, P),
                  'chain_pd': (torch.float64, C_, Fs, G, P), 'chain_draws': (torch.int64, C_, Fs)}
        out = {k: new(*shapes[k]) for k in self.PD_OUTPUTS if k in want}
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_predict_partial_dependence(self._h, _ptr(theta), C_, S_, _ptr(x), N, (C.c_int32 * Fs)(*feats), Fs,
                                                                _ptr(grid), G, int(max_draws_per_pass), int(max_rows_per_tile),
                                                                *[_ptr(out.get(k)) for k in self.PD_OUTPUTS], self._stream()), self.lib)
        return out

    def debug_quantile_sweeps(self):
        """(rows, total sweeps, most sweeps of a row) of the solver in the last ``predict_quantiles`` (test and tool hook)."""
        rows, total, most = C.c_int64(), C.c_int64(), C.c_int32()
        _lib.check(self.lib.mile_debug_quantile_sweeps(self._h, C.byref(rows), C.byref(total), C.byref(most)), self.lib)
        return int(rows.value), int(total.value), int(most.value)

    def lppd_stream_workspace(self, C: int, N: int) -> int:
        """Bytes of the (max, scaled sum) state and partial sums ``lppd_stream`` keeps for C chains on N rows, beyond the
        pass's block of log-likelihoods (mile_lppd_stream_workspace)."""
        return int(self.lib.mile_lppd_stream_workspace(self._h, int(C), int(N)))

    def lppd_stream(self, samples, x, y, curve_points=None, max_draws_per_pass: int = 0) -> dict:
        """LPPD of samples [C, S, d] on (x [N, F], y [N]) and its curves over the number of draws, reduced on the device
        (mile_lppd_stream) -- ``metrics.lppd`` and ``metrics.running_lppd`` of ``pointwise_loglik``'s [C, S, N] tensor without
        ever holding it, and without the underflow of exp(l).  ``curve_points``: increasing draw counts per chain in
        [1, S] (None: ``metrics.curve_points(S)``; empty: no curves).  Returns fp64 tensors on the device:
        ``curve_points`` [K] int32, ``run_chain`` [K] (the chain-averaged running LPPD), ``run_ens`` [K] (the LPPD of the
        first k draws of all chains), ``chain_lppd`` [C], ``row_lppd`` [N], ``lppd`` [] and ``dropped`` [C] int64, the (draw,
        row) pairs of each chain left out for a NaN log-likelihood.  ``max_draws_per_pass`` bounds the draws of each chain
        forwarded at a time (0: the library's choice); the outputs do not depend on it, bit for bit.  A host ``samples`` is
        uploaded whole: the library reads all chains' windows from one device array."""
        from mile_amd.metrics import curve_points as default_points
        samples = _f32(samples, self.device, name='samples')
        if samples.ndim != 3 or samples.shape[2] != self.d:
            raise ValueError(f'samples must be [C, S, {self.d}]')
        (C_, S_), theta, X, y = self._eval_inputs(samples, x, y, name_x='x')
        pts = default_points(S_) if curve_points is None else curve_points
        pts = torch.as_tensor(pts, dtype=torch.int32, device=self.device).reshape(-1).contiguous()
        K, N = int(pts.numel()), int(X.shape[0])
        f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.device)
        out = {'curve_points': pts, 'run_chain': f64(K), 'run_ens': f64(K), 'chain_lppd': f64(C_), 'row_lppd': f64(N),
               'lppd': f64(), 'dropped': torch.empty(C_, dtype=torch.int64, device=self.device)}
        curve = lambda k: _ptr(out[k]) if K else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_lppd_stream(self._h, _ptr(theta), C_, S_, _ptr(X), _ptr(y), N, _ptr(pts) if K else None, K,
                                                 curve('run_chain'), curve('run_ens'), _ptr(out['chain_lppd']),
                                                 _ptr(out['row_lppd']), _ptr(out['lppd']), _ptr(out['dropped']),
                                                 int(max_draws_per_pass), self._stream()), self.lib)
        return out

    def _loo_outputs(self, N, r_eff):
        r_eff = float(r_eff)                                               # (the library refuses one that is not finite and positive)
        out = {k: torch.empty(N, dtype=torch.float64, device=self.device) for k in ('lppd', 'p_waic', 'elpd_loo', 'khat')}
        out['dropped'] = torch.empty(N, dtype=torch.int32, device=self.device)
        return r_eff, out

    def psis_loo(self, loglik, r_eff: float = 1.0) -> dict:
        """PSIS-LOO and WAIC per row from pointwise log-likelihoods loglik [..., N] (every leading axis is a draw axis; from
        ``pointwise_loglik`` or anywhere else), by the library's kernels (mile_psis_loo): fp64 device tensors ``lppd``,
        ``p_waic``, ``elpd_loo``, ``khat`` [N] and ``dropped`` [N] int32 -- ``metrics.psis_loo`` of the same tensor.
        ``r_eff``: relative efficiency of the draws (1: independent).  ``metrics.loo_summary`` gives the totals."""
        ll = _f32(loglik, self.device, name='loglik')
        if ll.ndim < 2:
            raise ValueError('loglik must be [..., N]')
        N = int(ll.shape[-1])
        ll = ll.reshape(-1, N).contiguous()
        r_eff, out = self._loo_outputs(N, r_eff)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_psis_loo(_ptr(ll), ll.shape[0], N, r_eff, _ptr(out['lppd']), _ptr(out['p_waic']),
                                              _ptr(out['elpd_loo']), _ptr(out['khat']), _ptr(out['dropped']), self._stream()), self.lib)
        return out

    def loo_stream_workspace(self, S: int, N: int) -> int:
        """Bytes of the workspace ``loo_stream`` keeps in the handle for S draws on N rows with the library's own tile
        (mile_loo_stream_workspace)."""
        return int(self.lib.mile_loo_stream_workspace(self._h, int(S), int(N)))

    def loo_stream(self, theta, X, y, r_eff: float = 1.0, max_draws_per_pass: int = 0, max_rows_per_tile: int = 0) -> dict:
        """``psis_loo`` of ``pointwise_loglik``'s tensor for draws theta [..., d] on (X [N, F], y [N]) -- the rows the sampler
        conditioned on -- without ever holding it (mile_loo_stream): the rows go in tiles of at most ``max_rows_per_tile``
        (0: the library's choice), the forward inside a tile in passes of at most ``max_draws_per_pass`` draws (0: all).  The
        result does not depend on the two sizes, bit for bit."""
        _, th, X, y = self._eval_inputs(theta, X, y)
        N = int(X.shape[0])
        r_eff, out = self._loo_outputs(N, r_eff)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_loo_stream(self._h, _ptr(th), th.shape[0], _ptr(X), _ptr(y), N, r_eff, _ptr(out['lppd']),
                                                _ptr(out['p_waic']), _ptr(out['elpd_loo']), _ptr(out['khat']), _ptr(out['dropped']),
                                                int(max_draws_per_pass), int(max_rows_per_tile), self._stream()), self.lib)
        return out

    def chain_loo_stream_workspace(self, C_: int, S: int, N: int) -> int:
        """Bytes of the workspace ``chain_loo_stream`` keeps in the handle for C chains of S draws on N rows with the library's
        own tile (mile_chain_loo_stream_workspace): that of one chain."""
        return int(self.lib.mile_chain_loo_stream_workspace(self._h, int(C_), int(S), int(N)))

    def chain_loo_stream(self, samples, X, y, r_eff: float = 1.0, outputs=('lppd', 'p_waic', 'elpd_loo', 'khat', 'dropped'),
                         max_draws_per_pass: int = 0, max_rows_per_tile: int = 0) -> dict:
        """``loo_stream`` of every chain of samples [C, S, d] on its own (mile_chain_loo_stream): the ``outputs`` asked for, each
        [C, N] (fp64; ``dropped`` int32), row c bitwise what ``loo_stream(samples[c], ...)`` gives.  ``outputs=('lppd',)`` is the
        per-chain log predictive density of a held-out split, and ends each row after its first pass.  The result does not
        depend on the two sizes, bit for bit."""
        names = ('lppd', 'p_waic', 'elpd_loo', 'khat', 'dropped')
        outputs = tuple(outputs)
        if not outputs or any(k not in names for k in outputs):
            raise ValueError(f'outputs: a non-empty choice of {names}')
        samples = _f32(samples, self.device, name='samples')
        if samples.ndim != 3 or samples.shape[2] != self.d:
            raise ValueError(f'samples must be [C, S, {self.d}]')
        (C_, S_), th, X, y = self._eval_inputs(samples, X, y)
        N = int(X.shape[0])
        out = {k: torch.empty((C_, N), dtype=torch.int32 if k == 'dropped' else torch.float64, device=self.device) for k in outputs}
        ptr = lambda k: _ptr(out[k]) if k in out else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_chain_loo_stream(self._h, _ptr(th), C_, S_, _ptr(X), _ptr(y), N, float(r_eff), ptr('lppd'),
                                                      ptr('p_waic'), ptr('elpd_loo'), ptr('khat'), ptr('dropped'),
                                                      int(max_draws_per_pass), int(max_rows_per_tile), self._stream()), self.lib)
        return out

    LXP_OUTPUTS = ('expect', 'posterior', 'ess_w', 'khat', 'elpd_loo', 'dropped')

    def _lxp_outputs(self, outputs, names, N, Q, S):
        outputs = tuple(outputs)
        if not outputs or any(k not in names for k in outputs):
            raise ValueError(f'outputs: a non-empty choice of {names}')
        shapes = {'expect': (N, Q), 'posterior': (N, Q), 'weights': (N, S)}
        return {k: torch.empty(shapes.get(k, (N,)), dtype=torch.int32 if k == 'dropped' else torch.float64, device=self.device)
                for k in outputs}

    def psis_expect(self, loglik, values=None, r_eff: float = 1.0, outputs=None) -> dict:
        """PSIS-LOO expectations per row from pointwise log-likelihoods loglik [S, N] and per-draw columns values [S, N, Q]
        (fp32, from anywhere; Q <= 64), by the library's kernels (mile_psis_expect): of the ``outputs`` asked for, ``expect`` and
        ``posterior`` [N, Q] (sum_s w_s h and the in-sample mean), ``ess_w``, ``khat``, ``elpd_loo`` [N] (fp64), ``dropped`` [N]
        int32 and ``weights`` [N, S] fp64, the smoothed normalised weights in draw order -- ``metrics.psis_expect_dense`` of the
        same tensors.  ``outputs=None``: all but the weights, without ``expect`` and ``posterior`` where ``values`` is None."""
        ll = _f32(loglik, self.device, name='loglik')
        if ll.ndim != 2:
            raise ValueError('loglik must be [S, N]')
        ll = ll.contiguous()
        S_, N = int(ll.shape[0]), int(ll.shape[1])
        Q = 1
        if values is not None:
            values = _f32(values, self.device, name='values')
            if values.ndim == 2:
                values = values[:, :, None]
            if values.ndim != 3 or values.shape[:2] != ll.shape:
                raise ValueError('values must be [S, N, Q]')
            values = values.contiguous()
            Q = int(values.shape[2])
        if outputs is None:
            outputs = self.LXP_OUTPUTS if values is not None else self.LXP_OUTPUTS[2:]
        out = self._lxp_outputs(outputs, self.LXP_OUTPUTS + ('weights',), N, Q, S_)
        ptr = lambda k: _ptr(out[k]) if k in out else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_psis_expect(_ptr(ll), _ptr(values), S_, N, Q, float(r_eff), ptr('expect'), ptr('posterior'),
                                                 ptr('ess_w'), ptr('khat'), ptr('elpd_loo'), ptr('dropped'), ptr('weights'),
                                                 self._stream()), self.lib)
        return out

    def loo_predict_columns(self) -> int:
        """Columns of ``loo_predict_stream``'s ``expect``: 4 for regression (mu, mu^2, sigma^2, PIT), K for classification."""
        return 4 if self.spec.task == 'regr' else int(self.spec.hidden_structure[-1])

    def loo_predict_stream_workspace(self, S: int, N: int) -> int:
        """Bytes of the workspace ``loo_predict_stream`` keeps in the handle for S draws on N rows with the library's own tile
        (mile_loo_predict_stream_workspace); -1 where the call would be refused."""
        return int(self.lib.mile_loo_predict_stream_workspace(self._h, int(S), int(N)))

    def loo_predict_stream(self, theta, X, y, r_eff: float = 1.0, outputs=LXP_OUTPUTS, max_draws_per_pass: int = 0,
                           max_rows_per_tile: int = 0) -> dict:
        """Leave-one-out predictions for draws theta [..., d] on (X [N, F], y [N]), the rows the sampler conditioned on, from one
        forward per (draw, row) and without ever holding a per-draw tensor (mile_loo_predict_stream): ``expect`` [N, Q] =
        sum_s w_s h_q with the PSIS weights of ``loo_stream``'s l, for regression the columns (mu, mu^2, sigma^2,
        Phi((y - mu) / sigma)) -- LOO mean, second moment of the mean, aleatoric variance and LOO-PIT -- and for classification
        (K <= 64) the class probabilities; ``posterior`` [N, Q] their in-sample means; ``ess_w``, ``khat``, ``elpd_loo`` [N]
        (fp64) and ``dropped`` [N] int32.  The rows go in tiles of at most ``max_rows_per_tile`` (0: the library's choice), the
        forward in passes of at most ``max_draws_per_pass`` draws (0: all); the result does not depend on either, bit for bit."""
        _, th, X, y = self._eval_inputs(theta, X, y)
        N = int(X.shape[0])
        out = self._lxp_outputs(outputs, self.LXP_OUTPUTS, N, self.loo_predict_columns(), th.shape[0])
        ptr = lambda k: _ptr(out[k]) if k in out else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_loo_predict_stream(self._h, _ptr(th), th.shape[0], _ptr(X), _ptr(y), N, float(r_eff), ptr('expect'),
                                                        ptr('posterior'), ptr('ess_w'), ptr('khat'), ptr('elpd_loo'), ptr('dropped'),
                                                        int(max_draws_per_pass), int(max_rows_per_tile), self._stream()), self.lib)
        return out

    def stack_eval(self, lpd, w, outputs=('score', 'grad', 'hess', 'used'), max_rows_per_tile: int = 0) -> dict:
        """One evaluation of the stacking objective on the device (mile_stack_eval): lpd [C, N] and w [C] (fp64, entries >= 0)
        -> the ``outputs`` asked for among ``score`` [], ``row_score`` [N], ``grad`` [C], ``hess`` [C, C] (fp64) and ``used`` []
        int64, device tensors -- ``metrics.stack_eval_dense`` of the same inputs.  The result does not depend on
        ``max_rows_per_tile``, bit for bit.  A call without ``hess`` computes only what the rest needs."""
        names = ('score', 'row_score', 'grad', 'hess', 'used')
        outputs = tuple(outputs)
        if not outputs or any(k not in names for k in outputs):
            raise ValueError(f'outputs: a non-empty choice of {names}')
        lpd = torch.as_tensor(lpd).to(device=self.device, dtype=torch.float64).contiguous()
        if lpd.ndim != 2:
            raise ValueError('lpd must be [C, N]')
        C_, N = int(lpd.shape[0]), int(lpd.shape[1])
        w = torch.as_tensor(w).to(device=self.device, dtype=torch.float64).reshape(-1).contiguous()
        if w.shape != (C_,):
            raise ValueError('w must be [C]')
        shapes = {'score': (), 'row_score': (N,), 'grad': (C_,), 'hess': (C_, C_), 'used': ()}
        out = {k: torch.empty(shapes[k], dtype=torch.int64 if k == 'used' else torch.float64, device=self.device) for k in outputs}
        ptr = lambda k: _ptr(out[k]) if k in out else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_stack_eval(_ptr(lpd), _ptr(w), C_, N, ptr('score'), ptr('row_score'), ptr('grad'), ptr('hess'),
                                                ptr('used'), int(max_rows_per_tile), self._stream()), self.lib)
        return out

    def _crps_call(self, C_, N, y, weights, outputs):
        """What both CRPS methods share: y [N] fp32 on the device, the checked host weights and their pointer, the output
        tensors and a pointer getter."""
        from mile_amd.metrics import CRPS_OUTPUTS, crps_weights
        outputs = tuple(outputs)
        if not outputs or any(k not in CRPS_OUTPUTS for k in outputs):
            raise ValueError(f'outputs: a non-empty choice of {CRPS_OUTPUTS}')
        y = torch.as_tensor(y, device=self.device).to(torch.float32).reshape(-1).contiguous()
        if y.shape != (N,):
            raise ValueError('y must be [N]')
        W = crps_weights(weights, C_)
        n_w = int(W.shape[0])
        w_c = (C.c_double * max(1, n_w * C_))(*W.reshape(-1).tolist())
        shapes = {'crps_chain': (C_, N), 'spread_chain': (C_, N), 'crps_mix': (1 + n_w, N), 'spread_mix': (1 + n_w, N),
                  'gram': (N, C_, C_), 'dropped': (C_, N)}
        out = {k: torch.empty(shapes[k], dtype=torch.int32 if k == 'dropped' else torch.float64, device=self.device) for k in outputs}
        return y, (w_c if n_w else None), n_w, out, (lambda k: _ptr(out[k]) if k in out else None)

    def mixture_crps(self, raw, y, weights=None, outputs=('crps_chain', 'spread_chain', 'crps_mix', 'spread_mix', 'dropped'),
                     max_rows_per_tile: int = 0) -> dict:
        """The exact CRPS of the mixture of Normals that raw outputs [C, S, N, 2] (mu, log sigma) describe on each row, against
        y [N], by the library's pair kernel (mile_mixture_crps): the ``outputs`` asked for among ``crps_chain``,
        ``spread_chain`` [C, N] (every chain alone: its CRPS and half the expected distance of two of its draws), ``crps_mix``,
        ``spread_mix`` [1 + n_w, N] (row 0 the pooled ensemble of all kept draws, then the chain-weighted mixtures of
        ``weights`` [n_w, C] or [C], at most 8 vectors on the simplex), ``gram`` [N, C, C] (the mean pair term between chains,
        exactly symmetric) and ``dropped`` [C, N] int32 -- fp64 device tensors, ``metrics.mixture_crps_dense`` of the same
        inputs.  The raw outputs may come from anywhere -- ``predict``, or a deep ensemble's members as chains of one draw."""
        raw = _f32(raw, self.device, name='raw')
        if raw.ndim != 4 or raw.shape[-1] != 2:
            raise ValueError('raw must be [C, S, N, 2]')
        C_, S_, N = (int(v) for v in raw.shape[:3])
        r = raw.contiguous()
        y, w_c, n_w, out, ptr = self._crps_call(C_, N, y, weights, outputs)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_mixture_crps(_ptr(r), C_, S_, N, _ptr(y), w_c, n_w, ptr('crps_chain'), ptr('spread_chain'),
                                                  ptr('crps_mix'), ptr('spread_mix'), ptr('gram'), ptr('dropped'),
                                                  int(max_rows_per_tile), self._stream()), self.lib)
        return out

    def crps_stream_workspace(self, C_: int, S: int, N: int) -> int:
        """Bytes of the workspace ``crps_stream`` keeps in the handle for C chains of S draws on N rows with the library's own
        tile (mile_crps_stream_workspace)."""
        return int(self.lib.mile_crps_stream_workspace(self._h, int(C_), int(S), int(N)))

    def crps_stream(self, samples, X, y, weights=None, outputs=('crps_chain', 'spread_chain', 'crps_mix', 'spread_mix', 'dropped'),
                    max_draws_per_pass: int = 0, max_rows_per_tile: int = 0) -> dict:
        """``mixture_crps`` of ``predict``'s outputs for samples [C, S, d] on (X [N, F], y [N]) without ever holding them
        (mile_crps_stream): the rows go in tiles of at most ``max_rows_per_tile`` (0: the library's choice), the forward inside
        a tile in passes of at most ``max_draws_per_pass`` draws (0: all).  The result does not depend on the two sizes, bit
        for bit.  Regression only."""
        if self.spec.task != 'regr':
            raise ValueError('crps_stream: a regression model is needed')
        samples = _f32(samples, self.device, name='samples')
        if samples.ndim != 3 or samples.shape[2] != self.d:
            raise ValueError(f'samples must be [C, S, {self.d}]')
        (C_, S_), th, X, _ = self._eval_inputs(samples, X)
        N = int(X.shape[0])
        y, w_c, n_w, out, ptr = self._crps_call(C_, N, y, weights, outputs)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_crps_stream(self._h, _ptr(th), C_, S_, _ptr(X), _ptr(y), N, w_c, n_w, ptr('crps_chain'),
                                                 ptr('spread_chain'), ptr('crps_mix'), ptr('spread_mix'), ptr('gram'), ptr('dropped'),
                                                 int(max_draws_per_pass), int(max_rows_per_tile), self._stream()), self.lib)
        return out

    @staticmethod
    def _calibration_levels(coverages):
        lv = [float(v) for v in torch.as_tensor(coverages, dtype=torch.float64).reshape(-1)]
        if not 1 <= len(lv) <= 16:
            raise ValueError('coverages: between 1 and 16 of them')
        return (C.c_double * len(lv))(*lv), lv                          # (the library checks their range and order)

    def _calibration_outputs(self, G, N, K, lv, n_bins, y):
        dev, Q = self.device, len(lv)
        if y is not None:
            y = torch.as_tensor(y, device=dev).to(torch.int32).reshape(-1).contiguous()
            if y.shape != (N,):
                raise ValueError('y must be [N]')
        out = {'coverages': torch.tensor(lv, dtype=torch.float64, device=dev),
               'probs': torch.empty((G, N, K), dtype=torch.float64, device=dev),
               'kept': torch.empty((G, N), dtype=torch.int32, device=dev),
               'order': torch.empty((N, K), dtype=torch.int32, device=dev),
               'set_size': torch.empty((N, Q), dtype=torch.int32, device=dev)}
        if y is not None:
            out['rank'] = torch.empty(N, dtype=torch.int32, device=dev)
            out['totals'] = torch.empty((G, 5 + 2 * Q), dtype=torch.float64, device=dev)
            out['bins'] = torch.empty((G, max(int(n_bins), 0), 3), dtype=torch.float64, device=dev)
        ptrs = [_ptr(out.get(k)) for k in ('probs', 'kept', 'order', 'set_size', 'rank', 'totals', 'bins')]
        return y, out, ptrs

    def calibration(self, raw, y=None, coverages=(0.5, 0.75, 0.9, 0.95), n_bins: int = 15) -> dict:
        """Prediction sets and calibration of a classification ensemble from logits raw [C, S, N, K] (from ``predict``, or a deep
        ensemble's members with S = 1), by the library's kernels (mile_calibration), for every chain (groups 0 .. C - 1) and the
        ensemble of all chains (group C): device tensors ``probs`` [C + 1, N, K] fp64 (mean softmax of the draws whose logits
        are all finite on the row), ``kept`` [C + 1, N] int32, and of the ensemble ``order`` [N, K] (classes by descending
        probability, ties to the lower index) and ``set_size`` [N, Q] (the smallest highest-probability set whose sequential
        sum reaches each of ``coverages``) int32.  With labels ``y`` [N] also ``rank`` [N] (1-based position of the label in
        the order; 0 for a label outside [0, K)), ``totals`` [C + 1, 5 + 2 Q] (rows counted, rows correct, sum Brier, sum
        NLL, bad labels, rows covered per level, sum of set sizes per level) and ``bins`` [C + 1, n_bins, 3] (count, sum of
        confidence, sum of correct per equal-width confidence bin) fp64 -- ``metrics.classification_calibration`` of the same
        tensor; ``metrics.calibration_summary`` turns them into ACC, Brier, NLL, ECE, MCE, coverage and mean set size.
        K <= 64."""
        lvc, lv = self._calibration_levels(coverages)
        raw = _f32(raw, self.device, name='raw')
        if raw.ndim != 4:
            raise ValueError('raw must be [C, S, N, K]')
        C_, S_, N, K = (int(v) for v in raw.shape)
        r = raw.contiguous()
        y, out, ptrs = self._calibration_outputs(C_ + 1, N, K, lv, n_bins, y)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_calibration(_ptr(r), C_, S_, N, K, _ptr(y), lvc, len(lv), int(n_bins), *ptrs, self._stream()),
                       self.lib)
        return out

    def calibration_stream_workspace(self, C: int, S: int, N: int) -> int:
        """Upper bound of the bytes of the workspace ``calibration_stream`` keeps in the handle for C chains of S draws on N rows
        with the library's own tile and pass (mile_calibration_stream_workspace)."""
        return int(self.lib.mile_calibration_stream_workspace(self._h, int(C), int(S), int(N)))

    def calibration_stream(self, samples, x, y=None, coverages=(0.5, 0.75, 0.9, 0.95), n_bins: int = 15,
                           max_draws_per_pass: int = 0, max_rows_per_tile: int = 0) -> dict:
        """``calibration`` of ``predict``'s logits for samples [C, S, d] on x [N, F] without ever holding them
        (mile_calibration_stream): the rows go in tiles of at most ``max_rows_per_tile`` (0: the library's choice), the forward
        inside a tile in passes of at most ``max_draws_per_pass`` draws of every chain (0: the library's choice).  The result
        does not depend on the two sizes, bit for bit.  Classification only."""
        lvc, lv = self._calibration_levels(coverages)                   # (the library refuses a regression handle)
        samples = _f32(samples, self.device, name='samples')
        if samples.ndim != 3 or samples.shape[2] != self.d:
            raise ValueError(f'samples must be [C, S, {self.d}]')
        (C_, S_), theta, X, _ = self._eval_inputs(samples, x, name_x='x')
        N, K = int(X.shape[0]), int(self.spec.hidden_structure[-1])
        y, out, ptrs = self._calibration_outputs(C_ + 1, N, K, lv, n_bins, y)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_calibration_stream(self._h, _ptr(theta), C_, S_, _ptr(X), _ptr(y), N, lvc, len(lv), int(n_bins),
                                                        *ptrs, int(max_draws_per_pass), int(max_rows_per_tile), self._stream()),
                       self.lib)
        return out

    def function_diagnostics_workspace(self, C_: int, S: int, N: int, with_y: bool = True) -> int:
        """Bytes of the workspace ``function_diagnostics`` keeps in the handle for C chains of S draws on N rows with the
        library's own tile (mile_function_diagnostics_workspace); -1 out of range."""
        return int(self.lib.mile_function_diagnostics_workspace(self._h, int(C_), int(S), int(N), int(bool(with_y))))

    def function_diagnostics(self, samples, x, y=None, n_splits: int = 2, what=('wcv', 'bcv', 'ess', 'crhat', 'rhat'),
                             return_columns: bool = False, max_draws_per_pass: int = 0, max_rows_per_tile: int = 0) -> dict:
        """Chain diagnostics in function space (mile_function_diagnostics): ``metrics.chain_diagnostics`` of what samples
        [C, S, d] predict on x [N, F], without ever holding ``predict``'s tensor.  With O the head's width and Q = O + 1 (Q = O
        without ``y``), column n * Q + q is quantity q of row n -- regression: mu, log sigma, the row's log-likelihood;
        classification: the K softmax probabilities, the row's log-likelihood -- and with ``y`` the last column, M - 1 = N * Q,
        is the draw's summed log-likelihood.  ``what``: the statistics wanted.  Returns fp32 tensors on the device, None for
        what was not asked: ``wcv``, ``bcv``, ``rhat`` [M]; ``ess``, ``crhat`` [C, M]; ``columns`` [M, C, S] with
        ``return_columns``; ``loglik_sum`` [C, S] fp64 with ``y``; and, when ess, crhat and rhat are all in ``what``,
        ``summary`` (a dict keyed by ``_lib.FDIAG_SUMMARY`` over the N * Q per-row columns) and ``chain_summary`` [C, 2] fp64
        (each chain's min ess and max crhat); ``Q`` and ``M``.  No output depends on ``max_draws_per_pass`` or
        ``max_rows_per_tile`` (0: the library's choice), bit for bit.  ess / rhat need C * S <= 16384
        (``metrics.function_diagnostics`` goes on past that)."""
        samples = _f32(samples, self.device, name='samples')
        if samples.ndim != 3 or samples.shape[2] != self.d:
            raise ValueError(f'samples must be [C, S, {self.d}]')
        (C_, S_), theta, X, y = self._eval_inputs(samples, x, y, name_x='x')
        names = tuple(what)
        if any(k not in ('wcv', 'bcv', 'ess', 'crhat', 'rhat') for k in names):
            raise ValueError(f'what: names among wcv, bcv, ess, crhat, rhat, not {names}')
        bits = 0
        for k in names:
            bits |= _lib.DIAG_BITS[k]
        N, O = int(X.shape[0]), int(self.spec.hidden_structure[-1])
        Q = O + (1 if y is not None else 0)
        M = N * Q + (1 if y is not None else 0)
        new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=self.device)
        out = {k: (new(C_, M) if k in ('ess', 'crhat') else new(M)) if k in names else None for k in ('wcv', 'bcv', 'rhat', 'ess', 'crhat')}
        out['columns'] = new(M, C_, S_) if return_columns else None
        out['loglik_sum'] = new(C_, S_, dtype=torch.float64) if y is not None else None
        summed = all(k in names for k in ('ess', 'crhat', 'rhat'))
        summary = new(len(_lib.FDIAG_SUMMARY), dtype=torch.float64) if summed else None
        out['chain_summary'] = new(C_, 2, dtype=torch.float64) if summed else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_function_diagnostics(self._h, _ptr(theta), C_, S_, _ptr(X), _ptr(y), N, int(n_splits), bits,
                                                          _ptr(out['wcv']), _ptr(out['bcv']), _ptr(out['ess']), _ptr(out['crhat']),
                                                          _ptr(out['rhat']), _ptr(out['columns']), _ptr(out['loglik_sum']),
                                                          _ptr(summary), _ptr(out['chain_summary']), int(max_draws_per_pass),
                                                          int(max_rows_per_tile), self._stream()), self.lib)
        out['summary'] = dict(zip(_lib.FDIAG_SUMMARY, summary.cpu().tolist())) if summed else None
        out['Q'], out['M'] = Q, M
        return out

    def canonicalize(self, theta, key: str = 'bias', sign: bool = False, return_perm: bool = False):
        """theta [C, S, d] or [M, d] -> the canonical hidden-unit ordering of every draw on this engine's device
        (mile_amd.metrics.canonicalize with the engine's spec: mile_canonicalize_fcn)."""
        from mile_amd.metrics import canonicalize
        return canonicalize(self.spec, torch.as_tensor(theta).to(self.device, torch.float32), key, sign, return_perm)

    def align(self, theta, reference, sign: bool = False, return_index: bool = False, return_score: bool = False):
        """theta [C, S, d] or [M, d], reference [d] -> every draw with its hidden units matched to the reference's by assignment
        on this engine's device (one round of mile_amd.metrics.align with the engine's spec: mile_align_fcn).  With
        ``return_index`` also ``perm`` and ``sign`` [..., H], with ``return_score`` also ``score`` [..., n_hidden] fp64 and
        ``dropped`` [...] int32, in this order after the aligned draws."""
        from mile_amd.metrics import align
        res = align(self.spec, torch.as_tensor(theta).to(self.device, torch.float32),
                    torch.as_tensor(reference).to(self.device, torch.float32), 1, sign)
        out = (res['theta'],) + ((res['perm'], res['sign']) if return_index else ()) + ((res['score'], res['dropped']) if return_score else ())
        return out[0] if len(out) == 1 else out

    @property
    def supports_device_tuner(self) -> bool:
        return self.dim >= 4

    def debug_prefill_count(self) -> int:
        """Mid-step update launches so far whose E extra workgroups drew the record launch's noise (test hook)."""
        return int(self.lib.mile_debug_prefill_count(self._h))

    def debug_noise(self, seed: int, E: int, step: int, stage: int, particle_ids=None):
        ids = self._ids(particle_ids, E)
        out = torch.empty((E, self.dim), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.mile_debug_noise(self._h, C.c_uint64(seed), _ptr(ids), E, step, stage, _ptr(out),
                                                 self._stream()), self.lib)
        return out
