"""Per-leaf comparison of a gradient with its fp64 restatement, and the audit of what such a comparison can see.

A leaf is (name, begin, end) inside the raveled parameter vector.  The whole-vector criterion of DESIGN section 1
(`|g - g_ref|.max() < tol * |g_ref|.max()`) is set by the largest leaf -- with a narrow prior that is the prior's own gradient --
so a leaf whose likelihood gradient is smaller than the tolerance is not checked at all.  Here every leaf is held to its own
largest entry, chain by chain.
"""
from __future__ import annotations

import numpy as np

LEAF_TOL = 5e-5          # of the leaf's own largest entry (tests/test_gpu_lenet.py's per-leaf figure)
F32_MARGIN = 8.0         # a leaf may instead take this many times the float32 restatement's own error (summation order)


def spec_leaves(spec):
    """Leaves of a spec with `.leaves()` -> [(name, begin, end)]."""
    return [(n, int(o), int(o) + int(np.prod(s))) for n, o, s in spec.leaves()]


def fcn_leaves(ospec):
    """Leaves of an FCN oracle spec (oracle.param_slices) -> [(name, begin, end)], natural layer order."""
    from oracle import mclmc_oracle as M
    out = []
    for ent in M.param_slices(ospec):
        if ent['bias'] is not None:
            out.append((f"layer{ent['layer']}.bias", *ent['bias']))
        out.append((f"layer{ent['layer']}.kernel", *ent['kernel']))
    return out


def _2d(a):
    a = np.asarray(a, dtype=np.float64)
    return a[None] if a.ndim == 1 else a


def leaf_errors(g, g_ref, leaves, scale_of=None):
    """[E, n_leaves]: |g - g_ref|.max() over the leaf divided by |g_ref[leaf]|.max(), per chain.  `scale_of` maps a leaf name to
    the name of the leaf whose maximum scales it instead (for a leaf whose reference is zero analytically)."""
    g, g_ref = _2d(g), _2d(g_ref)
    assert g.shape == g_ref.shape, (g.shape, g_ref.shape)
    span = {n: (b, e) for n, b, e in leaves}
    out = np.zeros((g.shape[0], len(leaves)))
    for j, (n, b, e) in enumerate(leaves):
        sb, se = span[(scale_of or {}).get(n, n)]
        scale = np.abs(g_ref[:, sb:se]).max(axis=1)
        out[:, j] = np.abs(g[:, b:e] - g_ref[:, b:e]).max(axis=1) / np.maximum(scale, 1e-300)
    return out


def leaf_bounds(leaves, n_chains, g32=None, g_ref=None, scale_of=None, tol=LEAF_TOL, margin=F32_MARGIN):
    """[E, n_leaves] bound for leaf_errors: `tol`, or `margin` times the error of the float32 evaluation `g32` of the same
    restatement where that is larger (never anything taken from the code under test)."""
    bound = np.full((n_chains, len(leaves)), tol)
    if g32 is not None:
        bound = np.maximum(bound, margin * leaf_errors(g32, g_ref, leaves, scale_of))
    return bound


def assert_leaves(g, g_ref, leaves, bound=LEAF_TOL, scale_of=None, tag=None):
    """Every leaf of every chain within `bound` (a scalar or [E, n_leaves]) of its own largest reference entry; on failure reports
    the worst leaf, its chain, the index of the worst entry inside the leaf and every leaf that failed.  Returns the errors."""
    g, g_ref = _2d(g), _2d(g_ref)
    assert np.isfinite(g).all(), (tag, 'non-finite gradient')
    err = leaf_errors(g, g_ref, leaves, scale_of)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    bad = err >= bound
    if bad.any():
        ratio = np.where(bad, err / bound, 0.0)
        c, j = np.unravel_index(int(ratio.argmax()), ratio.shape)
        n, b, e = leaves[j]
        i = int(np.abs(g[c, b:e] - g_ref[c, b:e]).argmax())
        failed = sorted({leaves[jj][0] for jj in np.nonzero(bad.any(axis=0))[0]})
        raise AssertionError(f'{tag}: leaf {n!r} chain {c} index {i} (flat {b + i}): got {g[c, b + i]:.9g}, want {g_ref[c, b + i]:.9g}, '
                             f'error {err[c, j]:.3e} of the leaf maximum, bound {bound[c, j]:.3e}; failing leaves: {failed}')
    return err


def whole_vector_accepts(g, g_ref, tol=2e-5):
    """The criterion the per-leaf check stands next to: per chain, max |g - g_ref| < tol * max |g_ref|."""
    g, g_ref = _2d(g), _2d(g_ref)
    return bool((np.abs(g - g_ref).max(axis=1) < tol * np.abs(g_ref).max(axis=1)).all())


def visibility(g_lik_ref, g_ref, leaves, tol, per_leaf=True):
    """The "blind" ratio [E, n_leaves]: the absolute error a check admits on a leaf divided by the largest likelihood-gradient
    entry of that leaf.  >= 1: the kernel could write zero for that leaf's likelihood gradient and pass.  `per_leaf=True` is the
    per-leaf check (tol of the leaf's own maximum), False the whole-vector one (tol of the chain's maximum)."""
    g_lik_ref, g_ref = _2d(g_lik_ref), _2d(g_ref)
    out = np.zeros((g_ref.shape[0], len(leaves)))
    for j, (n, b, e) in enumerate(leaves):
        allowed = tol * (np.abs(g_ref[:, b:e]).max(axis=1) if per_leaf else np.abs(g_ref).max(axis=1))
        out[:, j] = allowed / np.maximum(np.abs(g_lik_ref[:, b:e]).max(axis=1), 1e-300)
    return out


def likelihood_share(g_lik_ref, g_ref, leaves):
    """[E, n_leaves]: max |likelihood gradient| / max |gradient| per leaf."""
    g_lik_ref, g_ref = _2d(g_lik_ref), _2d(g_ref)
    return np.stack([np.abs(g_lik_ref[:, b:e]).max(axis=1) / np.maximum(np.abs(g_ref[:, b:e]).max(axis=1), 1e-300)
                     for _, b, e in leaves], axis=1)


def table(names, values, fmt='%.2e'):
    """One line per leaf: name and the worst value over the chains (for the notes under profiles/)."""
    v = _2d(values).max(axis=0)
    return '\n'.join(f'  {n:<48s} {fmt % x}' for n, x in zip(names, v))
