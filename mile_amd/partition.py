"""Partition sampling layout (mirror of partition_params / merge_params, src/training/partition_sampling.py:304-315,157):
only the first and the last Dense layer of an FCN are sampled, every other layer keeps its chain's warm-start values.

The raveled order is lexicographic ('layer10' < 'layer2'), so the sampled coordinates are segments of the full row taken
from ``spec.leaves()``, never "head and tail".  The compact vector is those segments concatenated in full-row order.
Everything here is host-side layout arithmetic on numpy arrays or torch tensors; the library computes the same table
(mile_partition_segments) and Engine.set_partition checks the two against each other.
"""
from __future__ import annotations

import numpy as np

from mile_amd.spec import ModelSpec


def sampled_layers(spec) -> tuple:
    """Natural indices of the sampled layers: the first and the last; all of them when there are at most two."""
    n = len(spec.hidden_structure)
    return tuple(range(n)) if n <= 2 else (0, n - 1)


def check_spec(spec):
    if type(spec) is not ModelSpec:
        raise ValueError(f'partition sampling is built for the FCN only (first and last Dense layer), not for {type(spec).__name__}')


def segments(spec) -> list:
    """[(begin, length)] of the sampled coordinates inside the full row, in full-row order, adjacent leaves merged."""
    check_spec(spec)
    names = tuple(f'{spec.root}.layer{li}.' for li in sampled_layers(spec))
    segs = []
    for name, off, shape in spec.leaves():
        if not name.startswith(names):
            continue
        n = int(np.prod(shape))
        if segs and segs[-1][0] + segs[-1][1] == off:
            segs[-1] = (segs[-1][0], segs[-1][1] + n)
        else:
            segs.append((off, n))
    return segs


def sampled_index(spec) -> np.ndarray:
    """int64 [d_s]: the full-row index of every compact coordinate."""
    return np.concatenate([np.arange(b, b + n, dtype=np.int64) for b, n in segments(spec)])


def sampled_dim(spec) -> int:
    return sum(n for _, n in segments(spec))


def partition(spec, full):
    """full [..., d] -> compact [..., d_s] (numpy array or torch tensor)."""
    if full.shape[-1] != spec.n_params:
        raise ValueError(f'expected [..., {spec.n_params}], got {tuple(full.shape)}')
    idx = sampled_index(spec)
    if isinstance(full, np.ndarray):
        return full[..., idx]
    import torch
    return full[..., torch.as_tensor(idx, device=full.device)]


def merge(spec, compact, frozen):
    """compact [..., E, d_s] + frozen [E, d] -> full [..., E, d]: the frozen rows with their sampled coordinates replaced.
    The frozen coordinates of the result are copies of ``frozen``, bit for bit."""
    idx = sampled_index(spec)
    if compact.shape[-1] != len(idx) or frozen.shape[-1] != spec.n_params or compact.shape[-2] != frozen.shape[0]:
        raise ValueError(f'expected compact [..., E, {len(idx)}] and frozen [E, {spec.n_params}], got {tuple(compact.shape)} and '
                         f'{tuple(frozen.shape)}')
    lead = tuple(compact.shape[:-2])
    if isinstance(compact, np.ndarray):
        out = np.broadcast_to(frozen, lead + tuple(frozen.shape)).astype(compact.dtype, copy=True)
        out[..., idx] = compact
        return out
    import torch
    out = frozen.to(compact.dtype).expand(lead + tuple(frozen.shape)).clone()
    out[..., torch.as_tensor(idx, device=compact.device)] = compact
    return out
