"""Sampler plugin registry (mirror of src/training/kernels/__init__.py:14-20).

``KERNELS['mclmc']`` has blackjax.mclmc's factory shape:
    sampler = KERNELS['mclmc'](logdensity_fn, L=..., step_size=...)
    state = sampler.init(position, rng_key);  state, info = sampler.step(rng_key, state)
with every array carrying a leading ensemble axis (one row per chain), backed by
libmile_hip.so.  'mclmc_hip' is an alias.

``KERNELS['nuts']`` has blackjax.nuts's factory shape:
    sampler = KERNELS['nuts'](logdensity_fn, step_size, inverse_mass_matrix, max_num_doublings=10,
                              divergence_threshold=1000)
    state = sampler.init(position, rng_key);  state, info = sampler.step(rng_key, state)
(HMCState / NUTSInfo with the ensemble axis), backed by mile_nuts_step.  'hmc' stays unregistered: the reference has
no warm-up for it either.
"""
from __future__ import annotations

from typing import Callable, NamedTuple

import torch

from mile_amd.engine import HMCState, IntegratorState, MCLMCInfo, NUTSInfo
from mile_amd.probabilistic import is_partition_target, resolve_engine, resolve_target
from mile_amd.tree import as_key, ravel_tree

__all__ = ['mclmc', 'nuts', 'KERNELS', 'WARMUP_KERNELS', 'SamplingAlgorithm', 'HMCState', 'NUTSInfo']


class SamplingAlgorithm(NamedTuple):
    """blackjax.base.SamplingAlgorithm."""

    init: Callable
    step: Callable


def _flat(spec, position, device, eng=None):
    """[E, d] rows of a position; a partition engine gets their compact [E, d_s] form (full rows are cut down)."""
    flat = position if torch.is_tensor(position) else ravel_tree(spec, position)
    if flat.ndim == 1:
        flat = flat[None]
    flat = flat.to(device=device, dtype=torch.float32).contiguous()
    if eng is not None and eng.partitioned and eng.dim != eng.d and flat.shape[1] == eng.d:
        flat = eng.partition(flat)
    return flat


def mclmc(logdensity_fn, L, step_size, integrator: str = 'isokinetic_mclachlan', sqrt_diag_cov=1.0,
          chain_ids=None, refresh: str = 'O-step-O') -> SamplingAlgorithm:
    """blackjax.mclmc(logdensity_fn, L, step_size, integrator=isokinetic_mclachlan, sqrt_diag_cov=1.0)
    as called at src/training/sampling.py:133,173 (``config.kernel(unnorm_log_posterior, **parameters)``).

    L, step_size: scalars or [E] per-chain values (the reference tunes every chain separately,
    sampling.py:92-97).  chain_ids: global chain numbers keying the RNG streams.
    """
    if integrator != 'isokinetic_mclachlan':
        raise NotImplementedError('only the isokinetic McLachlan integrator is implemented')
    model, x, y = resolve_target(logdensity_fn)
    eng = resolve_engine(logdensity_fn)    # a partition target (ProbabilisticModel.bind_partition): compact states throughout
    sdc = None if (not torch.is_tensor(sqrt_diag_cov) and float(sqrt_diag_cov) == 1.0) else sqrt_diag_cov

    def init(position, rng_key) -> IntegratorState:
        key = as_key(rng_key)
        return eng.init(_flat(model.spec, position, eng.device, eng), seed=key.seed, particle_ids=chain_ids)

    def step(rng_key, state: IntegratorState, step_index: int = 0):
        """One kernel step.  The noise stream is Philox(rng_key.seed; chain id, step_index)."""
        key = as_key(rng_key)
        s = sdc
        if s is not None and torch.as_tensor(s).ndim < 2:
            s = torch.as_tensor(s, dtype=torch.float32, device=eng.device).expand(state.position.shape).contiguous()
        new, info, _ = eng.step(state, step_size, L, n_steps=1, seed=key.seed, step_offset=step_index,
                                particle_ids=chain_ids, refresh=refresh, sqrt_diag_cov=s)
        return new, MCLMCInfo(info.logdensity[0], info.kinetic_change[0], info.energy_change[0])

    return SamplingAlgorithm(init, step)


def nuts(logdensity_fn, step_size, inverse_mass_matrix, max_num_doublings: int = 10, divergence_threshold: float = 1000,
         chain_ids=None) -> SamplingAlgorithm:
    """blackjax.nuts(logdensity_fn, step_size, inverse_mass_matrix, max_num_doublings=10, divergence_threshold=1000) as
    built by sampler.get_kernel for sampler.name 'nuts' with the window-adapted parameters (src/training/sampling.py).

    step_size: scalar or [E]; inverse_mass_matrix: the diagonal, [d] or [E, d].  chain_ids: global chain numbers keying
    the RNG streams.
    """
    model, x, y = resolve_target(logdensity_fn)
    if is_partition_target(logdensity_fn):
        raise NotImplementedError('partition sampling with NUTS is not built yet')
    eng = model.engine(x, y)

    def init(position, rng_key=None) -> HMCState:
        return eng.nuts_init(_flat(model.spec, position, eng.device))

    def step(rng_key, state: HMCState, step_index: int = 0):
        """One NUTS step.  The draws are Philox(rng_key.seed; chain id, step_index)."""
        key = as_key(rng_key)
        new, info, _ = eng.nuts_step(state, step_size, inverse_mass_matrix, n_steps=1, max_num_doublings=max_num_doublings,
                                     divergence_threshold=divergence_threshold, seed=key.seed, step_offset=step_index,
                                     particle_ids=chain_ids)
        return new, NUTSInfo(*(f[0] for f in info))

    return SamplingAlgorithm(init, step)


KERNELS: dict[str, Callable[..., SamplingAlgorithm]] = {
    'mclmc': mclmc,
    'mclmc_hip': mclmc,
    'nuts': nuts,
}

WARMUP_KERNELS: dict[str, Callable[..., SamplingAlgorithm]] = {}
