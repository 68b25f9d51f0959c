"""fp64 restatement of blackjax 1.2.2 NUTS (nuts.build_kernel, velocity_verlet, diagonal metrics.default_metric) and of
its window adaptation (adaptation.window_adaptation.base / build_schedule), one chain at a time, written from the
blackjax sources' structure for the tests: it is the yardstick of mile_nuts_step / mile_nuts_warmup.

Random draws are explicit and use the library's slot layout (include/mile_hip.h, mile_nuts_args): for one step,
``z`` [d] momentum normals and ``u`` [2 M + 2^M] uniforms -- u[j] direction of doubling j (forward when < 0.5),
u[M + j] biased sampling of doubling j, u[2 M + n] uniform sampling of the n-th leaf of the step.
"""
from __future__ import annotations

import math
from typing import Callable, NamedTuple

import numpy as np


class HMCState(NamedTuple):
    position: np.ndarray
    logdensity: float
    logdensity_grad: np.ndarray


class NUTSInfo(NamedTuple):
    num_integration_steps: int
    acceptance_rate: float
    num_trajectory_expansions: int
    is_divergent: bool
    energy: float
    is_turning: bool


def logaddexp(a, b):
    return float(np.logaddexp(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# metrics.default_metric (diagonal)
def is_turning(m, p_left, p_right, p_sum):
    """gaussian_euclidean check_turning: rho = p_sum - (p_right + p_left) / 2, turning when either end's velocity points
    against rho."""
    rho = p_sum - 0.5 * (p_right + p_left)
    return bool(np.dot(m * p_left, rho) <= 0 or np.dot(m * p_right, rho) <= 0)


def kinetic(m, p):
    return 0.5 * float(np.dot(m * p, p))


# termination.iterative_uturn_numpyro
def leaf_idx_to_ckpt_idxs(n: int):
    idx_max = bin(n >> 1).count('1')
    num_subtrees = 0
    t = n
    while t & 1:
        num_subtrees += 1
        t >>= 1
    return idx_max - num_subtrees + 1, idx_max


class IterativeUTurn:
    def __init__(self, M, d):
        self.r = np.zeros((M, d))
        self.rs = np.zeros((M, d))
        self.idx_min = self.idx_max = 0

    def update(self, p_sum, p, step):
        self.idx_min, self.idx_max = leaf_idx_to_ckpt_idxs(step)
        if step % 2 == 0:
            self.r[self.idx_max] = p
            self.rs[self.idx_max] = p_sum

    def met(self, m, p_sum, p):
        for i in range(self.idx_max, self.idx_min - 1, -1):
            if is_turning(m, self.r[i], p, p_sum - self.rs[i] + self.r[i]):
                return True
        return False


class _Leaf(NamedTuple):
    x: np.ndarray
    p: np.ndarray
    logp: float
    g: np.ndarray


class _Proposal(NamedTuple):
    state: _Leaf
    energy: float
    weight: float
    sum_log_p_accept: float


def velocity_verlet(f: Callable, m, s: _Leaf, h: float) -> _Leaf:
    p = s.p + 0.5 * h * s.g
    x = s.x + h * m * p
    logp, g = f(x)
    return _Leaf(x, p + 0.5 * h * g, logp, g)


def nuts_step(f: Callable, state: HMCState, step_size: float, m, z, u, max_num_doublings: int = 10,
              divergence_threshold: float = 1000.0, trace=None):
    """One nuts.build_kernel step.  f(x) -> (logp, grad) in fp64; m the diagonal inverse mass matrix."""
    M = max_num_doublings
    m = np.asarray(m, dtype=np.float64)
    p0 = np.asarray(z, dtype=np.float64) / np.sqrt(m)                    # sample_momentum
    init = _Leaf(state.position, p0, state.logdensity, state.logdensity_grad)
    e0 = -init.logp + kinetic(m, p0)
    proposal = _Proposal(init, e0, 0.0, -np.inf)
    left = right = init
    p_sum = p0.copy()
    n_states = 0
    term = IterativeUTurn(M, p0.size)
    depth = 0
    is_div = is_turn = False
    while depth < M:
        direction = 1 if u[depth] < 0.5 else -1
        start = right if direction > 0 else left
        # trajectory.dynamic_progressive_integration, 2^depth leaves at most
        h = direction * step_size
        cur = start
        sub_prop = None
        sub_sum = None
        div = turn_sub = False
        k = 0
        while k < 2 ** depth:
            cur = velocity_verlet(f, m, cur, h)
            energy = -cur.logp + kinetic(m, cur.p)
            w = e0 - energy                                              # proposal_generator
            if math.isnan(w):
                w = -np.inf
            leaf_prop = _Proposal(cur, energy, w, min(w, 0.0))
            div = -w > divergence_threshold
            if k == 0:
                sub_prop = leaf_prop
                sub_sum = cur.p.copy()
            else:                                                        # progressive_uniform_sampling
                with np.errstate(invalid='ignore', over='ignore'):
                    pa = 1.0 / (1.0 + np.exp(-(w - sub_prop.weight)))
                acc = u[2 * M + n_states + k] < pa
                nw = logaddexp(sub_prop.weight, w)
                ns = logaddexp(sub_prop.sum_log_p_accept, leaf_prop.sum_log_p_accept)
                sub_prop = _Proposal(cur if acc else sub_prop.state, energy if acc else sub_prop.energy, nw, ns)
                sub_sum = sub_sum + cur.p
            term.update(sub_sum, cur.p, k)
            turn_sub = term.met(m, sub_sum, cur.p)
            k += 1
            if div or turn_sub:
                break
        if direction > 0:
            right = cur
        else:
            left = cur
        # dynamic_multiplicative_expansion: biased sampling unless the subtree diverged or turned
        if not (div or turn_sub):
            with np.errstate(over='ignore', invalid='ignore'):
                pa = min(np.exp(sub_prop.weight - proposal.weight), 1.0) if not math.isnan(sub_prop.weight - proposal.weight) else np.nan
            acc = u[M + depth] < pa
            proposal = _Proposal(sub_prop.state if acc else proposal.state, sub_prop.energy if acc else proposal.energy,
                                 logaddexp(proposal.weight, sub_prop.weight),
                                 logaddexp(proposal.sum_log_p_accept, sub_prop.sum_log_p_accept))
        else:
            proposal = proposal._replace(sum_log_p_accept=logaddexp(proposal.sum_log_p_accept, sub_prop.sum_log_p_accept))
        p_sum = p_sum + sub_sum
        n_states += k
        turn_full = is_turning(m, left.p, right.p, p_sum)
        depth += 1
        is_div, is_turn = div, turn_sub or turn_full
        if trace is not None:
            trace.append((depth, k, div, turn_sub, turn_full))
        if is_div or is_turn:
            break
    s = proposal.state
    info = NUTSInfo(n_states, math.exp(proposal.sum_log_p_accept) / n_states, depth, bool(is_div), proposal.energy,
                    bool(is_turn))
    return HMCState(s.x, s.logp, s.g), info


# ---------------------------------------------------------------------------------------------------------------------
# Recursive tree doubling (Hoffman & Gelman's BuildTree with the numpyro / blackjax turning criterion): the independent
# check of the iterative checkpoint algebra.  Returns the number of leaves built before a sub-tree turns, for a fixed
# sequence of momenta.
def recursive_subtree_turns(m, ps, depth):
    """Leaves [0, 2^depth) with momenta ps; returns the index of the leaf at which the iterative scheme must stop (the
    first leaf that completes a turning sub-sub-tree), or None."""
    stop = [None]

    def build(lo, hi):   # [lo, hi): returns (p_left, p_right, p_sum); records the completion index of a turn
        if hi - lo == 1:
            return ps[lo], ps[lo], ps[lo].copy()
        mid = (lo + hi) // 2
        a = build(lo, mid)
        if stop[0] is not None:
            return a
        b = build(mid, hi)
        if stop[0] is not None:
            return b
        tot = (a[0], b[1], a[2] + b[2])
        if is_turning(m, tot[0], tot[1], tot[2]):
            stop[0] = hi - 1
        return tot

    build(0, 2 ** depth)
    return stop[0]


def iterative_subtree_turns(m, ps, depth):
    term = IterativeUTurn(max(depth, 1) + 1, ps.shape[1])
    s = None
    for k in range(2 ** depth):
        s = ps[k].copy() if k == 0 else s + ps[k]
        term.update(s, ps[k], k)
        if term.met(m, s, ps[k]):
            return k
    return None


# ---------------------------------------------------------------------------------------------------------------------
# adaptation.window_adaptation
def build_schedule(num_steps, initial_buffer_size=75, final_buffer_size=50, first_window_size=25):
    num_steps = int(num_steps)
    if num_steps < 20:
        return np.array([(0, False)] * num_steps, dtype=np.int64).reshape(-1, 2)
    if initial_buffer_size + first_window_size + final_buffer_size > num_steps:
        initial_buffer_size = int(0.15 * num_steps)
        final_buffer_size = int(0.1 * num_steps)
        first_window_size = num_steps - (initial_buffer_size + final_buffer_size)
    schedule = [(0, False)] * initial_buffer_size
    final_window_start = num_steps - final_buffer_size
    next_size, next_start = first_window_size, initial_buffer_size
    while next_start < final_window_start:
        cur_start, cur_size = next_start, next_size
        if 3 * cur_size <= final_window_start - cur_start:
            next_size = 2 * cur_size
        else:
            cur_size = final_window_start - cur_start
        next_start = cur_start + cur_size
        schedule += [(1, False)] * (next_start - 1 - cur_start)
        schedule.append((1, True))
    schedule += [(0, False)] * (num_steps - final_window_start)
    return np.array(schedule, dtype=np.int64)


class DualAveraging:
    """optimizers.dual_averaging(t0=10, gamma=0.05, kappa=0.75) driven by target - acceptance_rate."""

    def __init__(self, step_size, t0=10.0, gamma=0.05, kappa=0.75):
        self.t0, self.gamma, self.kappa = t0, gamma, kappa
        self.reset(step_size)

    def reset(self, step_size):
        self.log_x, self.log_x_avg, self.step, self.avg_grad = math.log(step_size), 0.0, 1, 0.0
        self.mu = math.log(10 * step_size)

    def update(self, gradient):
        reg = self.step + self.t0
        eta = self.step ** (-self.kappa)
        self.avg_grad = (1 - 1 / reg) * self.avg_grad + gradient / reg
        self.log_x = self.mu - math.sqrt(self.step) / self.gamma * self.avg_grad
        self.log_x_avg = eta * self.log_x + (1 - eta) * self.log_x_avg
        self.step += 1


class WindowAdaptation:
    """window_adaptation.base(is_mass_matrix_diagonal=True, target_acceptance_rate) per chain."""

    def __init__(self, d, initial_step_size=1.0, target=0.8):
        self.target = target
        self.da = DualAveraging(initial_step_size)
        self.step_size = initial_step_size
        self.imm = np.ones(d)
        self._wreset(d)

    def _wreset(self, d):
        self.mean, self.m2, self.n = np.zeros(d), np.zeros(d), 0

    def update(self, stage, window_end, position, acceptance_rate):
        if stage == 1:                                    # slow_update: Welford
            self.n += 1
            delta = position - self.mean
            self.mean = self.mean + delta / self.n
            self.m2 = self.m2 + delta * (position - self.mean)
        self.da.update(self.target - acceptance_rate)
        self.step_size = math.exp(self.da.log_x)
        if window_end:                                    # slow_final
            n = self.n
            var = self.m2 / (n - 1)
            self.imm = (n / (n + 5.0)) * var + 1e-3 * (5.0 / (n + 5.0))
            self._wreset(position.size)
            self.da.reset(math.exp(self.da.log_x_avg))
            self.step_size = math.exp(self.da.log_x)

    def final(self):
        return math.exp(self.da.log_x_avg), self.imm
