"""fp64 NumPy restatement of the LeNetti target -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

LeNettiCore (src/models/images/cnns.py:69-121):
    x NCHW -> NHWC; Conv(1, 3x3, stride 1, padding 2) -> act -> flatten NHWC ((H+2)(W+2) features, index h*(W+2) + w)
    -> Dense(8) -> act -> Dense(8) -> act -> Dense(8) -> act -> Dense(out_dim)
flax nn.Conv is a cross-correlation with kernel [kh, kw, in, out] and a bias.  Likelihood and prior as for every other
target (oracle/mclmc_oracle.py: pointwise_loglik, log_prior).  Raveled parameter order = ravel_pytree's sorted keys of
{'core': {conv1, fc1, fc2, fc3, fc4}}, bias before kernel inside each.

Same signatures as oracle/lenet_oracle.py, so oracle.mclmc_init / mclmc_step, oracle.pointwise_loglik_raw and
tests/nuts_ref.nuts_step take `logpost_and_grad` as their log-density.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import mclmc_oracle as M


@dataclass(frozen=True)
class LeNettiSpec:
    channels: int
    height: int
    width: int
    out_dim: int
    activation: str = 'relu'
    task: str = 'classification'
    prior: str = 'Normal'
    prior_loc: float = 0.0
    prior_scale: float = 1.0

    def __post_init__(self):
        assert self.activation in M.ACTIVATIONS and self.task in M.TASKS and self.prior in M.PRIORS

    Ho = property(lambda s: s.height + 2)
    Wo = property(lambda s: s.width + 2)
    pixels = property(lambda s: s.Ho * s.Wo)
    in_features = property(lambda s: s.channels * s.height * s.width)

    def leaves(self):
        """[(dotted name, offset, shape)] in ravel_pytree order."""
        shapes = [('core.conv1.bias', (1,)), ('core.conv1.kernel', (3, 3, self.channels, 1)),
                  ('core.fc1.bias', (8,)), ('core.fc1.kernel', (self.pixels, 8)),
                  ('core.fc2.bias', (8,)), ('core.fc2.kernel', (8, 8)),
                  ('core.fc3.bias', (8,)), ('core.fc3.kernel', (8, 8)),
                  ('core.fc4.bias', (self.out_dim,)), ('core.fc4.kernel', (8, self.out_dim))]
        out, off = [], 0
        for n, sh in shapes:
            out.append((n, off, sh))
            off += int(np.prod(sh))
        return out

    @property
    def n_params(self) -> int:
        n, o, sh = self.leaves()[-1]
        return o + int(np.prod(sh))


def _unravel(spec: LeNettiSpec, theta: np.ndarray) -> dict:
    return {n: theta[:, o:o + int(np.prod(sh))].reshape((theta.shape[0],) + sh) for n, o, sh in spec.leaves()}


def _patches(X: np.ndarray, dt) -> np.ndarray:
    """[N, C, H, W] -> zero-padded NHWC 3x3 patches [N, P, 9*C] with column order (kh, kw, c) = the kernel's ravel order."""
    x = np.pad(np.transpose(X.astype(dt), (0, 2, 3, 1)), ((0, 0), (2, 2), (2, 2), (0, 0)))
    v = np.lib.stride_tricks.sliding_window_view(x, (3, 3), axis=(1, 2))          # [N, Ho, Wo, C, 3, 3]
    v = np.moveaxis(v, 3, -1)                                                       # [N, Ho, Wo, 3, 3, C]
    return v.reshape(X.shape[0], (X.shape[2] + 2) * (X.shape[3] + 2), -1)


def forward(spec: LeNettiSpec, theta: np.ndarray, X: np.ndarray, keep: bool = False):
    """theta [E, d], X [N, C, H, W] -> out [E, N, out_dim] (and the intermediates for the backward pass)."""
    P = _unravel(spec, theta)
    E = theta.shape[0]
    col = _patches(X, theta.dtype)                                                  # [N, P, 9C]
    z0 = np.einsum('npk,ek->enp', col, P['core.conv1.kernel'].reshape(E, -1)) + P['core.conv1.bias'][:, :, None]
    a0 = M._act(spec.activation, z0)                                                # [E, N, P]
    zs, hs, h = [], [a0], a0
    for name in ('fc1', 'fc2', 'fc3'):
        z = h @ P[f'core.{name}.kernel'] + P[f'core.{name}.bias'][:, None, :]
        h = M._act(spec.activation, z)
        zs.append(z)
        hs.append(h)
    out = h @ P['core.fc4.kernel'] + P['core.fc4.bias'][:, None, :]
    if keep:
        return out, dict(P=P, col=col, z0=z0, zs=zs, hs=hs)
    return out


def logpost_and_grad(spec: LeNettiSpec, theta: np.ndarray, X: np.ndarray, y: np.ndarray):
    """log_unnormalized_posterior and its gradient for an ensemble: theta [E, d] -> (logp [E], grad [E, d])."""
    E = theta.shape[0]
    out, c = forward(spec, theta, X, keep=True)
    P, hs, zs = c['P'], c['hs'], c['zs']
    ll, dout = M.pointwise_loglik(spec, out, y)
    lp, gp = M.log_prior(spec, theta)
    g = {'core.fc4.kernel': np.swapaxes(hs[3], 1, 2) @ dout, 'core.fc4.bias': dout.sum(axis=1)}
    dz = dout
    for li, name, nxt in ((2, 'fc3', 'fc4'), (1, 'fc2', 'fc3'), (0, 'fc1', 'fc2')):
        dz = (dz @ np.swapaxes(P[f'core.{nxt}.kernel'], 1, 2)) * M._act_grad(spec.activation, zs[li], hs[li + 1])
        g[f'core.{name}.kernel'] = np.swapaxes(hs[li], 1, 2) @ dz
        g[f'core.{name}.bias'] = dz.sum(axis=1)
    dz0 = (dz @ np.swapaxes(P['core.fc1.kernel'], 1, 2)) * M._act_grad(spec.activation, c['z0'], hs[0])   # [E, N, P]
    g['core.conv1.kernel'] = np.einsum('npk,enp->ek', c['col'], dz0).reshape(E, 3, 3, spec.channels, 1)
    g['core.conv1.bias'] = dz0.sum(axis=(1, 2))[:, None]
    grad = np.concatenate([g[n].reshape(E, -1) for n, _, _ in spec.leaves()], axis=1)
    return (lp + ll.sum(axis=-1)).astype(theta.dtype), (grad + gp).astype(theta.dtype)


def synthetic_problem(spec: LeNettiSpec, N: int, E: int, seed: int = 0) -> dict:
    """Seeded synthetic images/labels and flax-style initial parameters (lecun-normal kernels, small biases)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    X = rng.standard_normal((N, spec.channels, spec.height, spec.width)).astype(np.float32)
    if spec.task == 'classification':
        y = rng.integers(0, spec.out_dim, N).astype(np.int32)
    else:
        y = rng.standard_normal(N).astype(np.float32)
    theta = np.zeros((E, spec.n_params), dtype=np.float32)
    for n, o, sh in spec.leaves():
        k = int(np.prod(sh))
        if n.endswith('kernel'):
            theta[:, o:o + k] = rng.standard_normal((E, k)) / np.sqrt(int(np.prod(sh[:-1])))
        else:
            theta[:, o:o + k] = 0.05 * rng.standard_normal((E, k))
    d = spec.n_params
    return {'X': X, 'y': y, 'theta0': theta, 'u0': rng.standard_normal((E, d)).astype(np.float32),
            'eps': (1e-3 * (1 + 0.05 * rng.uniform(-1, 1, E))).astype(np.float32),
            'L': (np.sqrt(d) * 1e-2 * (1 + 0.05 * rng.uniform(-1, 1, E))).astype(np.float32)}
