"""Fitted Q evaluation in NumPy, written from the algorithm, and the case lists tests/test_fqe_ref.py (CPU) and tests/test_hip_fqe.py
(GPU) share.  Every function takes the dtype it computes in: float64 is the reference, float32 shows what a correct fp32
implementation reaches.

  y = r + gamma not_done 0.5 (Qt_1 + Qt_2)(s', pi(s'));  L = mse(Q_1(s, a), y) + mse(Q_2(s, a), y);  Adam (torch's defaults);
  Q_targ <- tau Q + (1 - tau) Q_targ;  the estimate is the mean over start states of 0.5 (Q_1 + Q_2)(s0, pi(s0)).
Policy heads: 0 a deterministic actor S -> A, action max_action tanh(z); 1 a Gaussian policy S -> 2 A, action max_action tanh(z[:, :A]).
"""
import numpy as np

import bosa_graph_cases as GC

TARGET_SHAPES = ((17, 6), (11, 3), (3, 1), (111, 8), (45, 24))          # (S, A)
TARGET_ROWS = (2, 33, 256, 257, 1025)     # 256 | 257: a workgroup's last thread and the next one's first; 1025: more than four workgroups
VALUE_ROWS = (1, 2, 255, 256, 257, 1025)  # one row per thread up to 256, then a second trip of the reducer's threads
HEADS = (0, 1)
MAX_ACTIONS = (1.0, 2.0)
STEP_BS = (8, 33)
TRAJ = dict(S=17, A=6, bs=33, steps=20, rows=500, gamma=0.99, tau=0.005, lr=3e-4, seed=3)
# constant rewards: r = 1, not_done = 1, gamma 0.9, so Q = 1 / (1 - gamma) = 10 whatever the state.  lr and tau are chosen so that
# CONST["steps"] steps reach 2 % in the fp64 restatement (tests/test_fqe_ref.py measures it); the GPU test allows 5 %.
CONST = dict(S=3, A=1, bs=32, rows=200, gamma=0.9, tau=0.05, lr=1e-3, steps=1000, seed=5)      # measured: 9.926 after 1000 steps (0.74 %)
# What the float32 NumPy restatement differs from the fp64 one after TRAJ's 20 steps, per policy head: the largest difference of a
# parameter, of a target parameter and of one of value()'s four words (measured by tests/test_fqe_ref.py, which holds a run to twice
# these).  The GPU trajectory test's tolerance is 4 x these.
TRAJ_F32_DIFF = {0: dict(param=1.72e-6, targ=1.59e-7, value=4.9e-8), 1: dict(param=3.93e-7, targ=1.06e-7, value=5.2e-8)}
SEED_FQE_INDEX, GATHER_STREAM = 111, 3    # fqe.SEED_FQE_INDEX; the stream id of the ring gather's index draws


def round4(n):
    return (n + 3) // 4 * 4


def workspace_floats(head, A, rows):
    """mobody_fqe_target_workspace / mobody_fqe_value_workspace: a' [rows][A], the twin Q [2][rows] and, for head 1, the policy's
    [rows][2 A] outputs, each piece rounded up to 4 floats."""
    return round4(rows * A) + round4(2 * rows) + (round4(rows * 2 * A) if head == 1 else 0)


def policy_params(seed, head, S, A):
    return GC.mlp_params(seed, S, A if head == 0 else 2 * A, 1)


def action(policy, head, A, s, ma, dtype=np.float64):
    z = GC.mlp(policy[0], s, dtype)
    return (dtype(np.float32(ma)) * np.tanh(z))[:, :A]


def twin_q(q, s, a, dtype=np.float64):
    x = np.concatenate([s.astype(dtype), a.astype(dtype)], 1)
    return np.stack([GC.mlp(p, x, dtype)[:, 0] for p in q])


def q_next(policy, head, A, q_targ, s2, ma, dtype=np.float64):
    a2 = action(policy, head, A, s2, ma, dtype)
    q = twin_q(q_targ, s2, a2, dtype)
    return (q[0] + q[1]) * dtype(0.5), a2


def value_words(q, dtype=np.float64):
    """(mean q0, mean q1, mean 0.5 (q0 + q1), max |q0 - q1|) of q [2][B]."""
    q = q.astype(dtype)
    return np.array([q[0].mean(), q[1].mean(), ((q[0] + q[1]) * dtype(0.5)).mean(), np.abs(q[0] - q[1]).max()], dtype)


def mean_tolerance(q):
    """Bound of the three fp32 means of q [2][B] against fp64 means of the same values: thread t adds its ceil(B / 256) rows in order,
    a tree of 8 levels joins the partial sums, one division: (ceil(B / 256) + 8) 2^-24 mean|q| (mean|q| over the rows the word
    averages; both members' rows for the third word)."""
    B = q.shape[1]
    k = (-(-B // 256) + 8) * 2.0 ** -24
    a = np.abs(q.astype(np.float64))
    return k * np.array([a[0].mean(), a[1].mean(), a.mean()])


class Fqe(object):
    """FQE's state and step in `dtype`: q, q_targ lists of per-member parameter lists (GC.mlp_params' layout), Adam moments, count."""

    def __init__(self, q, policy, head, A, ma, gamma, tau, lr, dtype=np.float64):
        self.dtype, self.head, self.A, self.ma = dtype, head, A, ma
        self.gamma, self.tau, self.lr = dtype(np.float32(gamma)), dtype(np.float32(tau)), float(np.float32(lr))
        self.policy = policy
        self.q = [[t.astype(dtype) for t in p] for p in q]
        self.q_targ = [[t.copy() for t in p] for p in self.q]
        self.m = [[np.zeros_like(t) for t in p] for p in self.q]
        self.v = [[np.zeros_like(t) for t in p] for p in self.q]
        self.t, self.loss = 0, None

    def step(self, s, a, s2, r, nd):
        dt = self.dtype
        qn, _ = q_next(self.policy, self.head, self.A, self.q_targ, s2, self.ma, dt)
        y = r.astype(dt).reshape(-1) + nd.astype(dt).reshape(-1) * self.gamma * qn
        x = np.concatenate([s.astype(dt), a.astype(dt)], 1)
        N = x.shape[0]
        self.t += 1
        b1, b2, eps = 0.9, 0.999, 1e-8
        c1, c2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        loss = dt(0)
        for k, p in enumerate(self.q):
            W1, bb1, W2, bb2, W3, bb3 = p
            z1 = x @ W1.T + bb1
            h1 = np.maximum(z1, 0)
            z2 = h1 @ W2.T + bb2
            h2 = np.maximum(z2, 0)
            q = (h2 @ W3.T + bb3)[:, 0]
            d = q - y
            loss = loss + (d * d).mean()
            dz3 = (dt(2) * d / dt(N))[:, None]
            dz2 = (dz3 @ W3) * (z2 > 0)
            dz1 = (dz2 @ W2) * (z1 > 0)
            grads = [dz1.T @ x, dz1.sum(0), dz2.T @ h1, dz2.sum(0), dz3.T @ h2, dz3.sum(0)]
            for j, g in enumerate(grads):
                g = g.astype(dt)
                self.m[k][j] = (dt(b1) * self.m[k][j] + dt(1 - b1) * g).astype(dt)
                self.v[k][j] = (dt(b2) * self.v[k][j] + dt(1 - b2) * g * g).astype(dt)
                denom = np.sqrt(self.v[k][j]) / dt(np.sqrt(c2)) + dt(eps)
                p[j] = (p[j] - dt(self.lr / c1) * self.m[k][j] / denom).astype(dt)
                self.q_targ[k][j] = (self.tau * p[j] + (dt(1) - self.tau) * self.q_targ[k][j]).astype(dt)
        self.loss = loss
        return loss

    def value(self, s0):
        a0 = action(self.policy, self.head, self.A, s0, self.ma, self.dtype)
        return value_words(twin_q(self.q, s0, a0, self.dtype), self.dtype)

    def flat(self, which="q"):
        return np.concatenate([t.reshape(-1).astype(np.float64) for p in getattr(self, which) for t in p])


def params_from_state_dict(sd):
    """GC.mlp_params' layout of a twin-Q state dict (nn.Linear names under network1. / network2.)."""
    return [[np.asarray(sd[f"{pre}network.{li}.{wb}"], np.float32) for li in (0, 2, 4) for wb in ("weight", "bias")]
            for pre in ("network1.", "network2.")]


def dataset(rows, S, A, seed, const_reward=False):
    """Target transitions (state, action, next_state, reward, not_done) in fp32: one long episode with a terminal every 50 rows."""
    rng = np.random.default_rng(9000 + seed)
    s = rng.standard_normal((rows, S)).astype(np.float32)
    a = rng.uniform(-1, 1, (rows, A)).astype(np.float32)
    s2 = (s + 0.1 * rng.standard_normal((rows, S))).astype(np.float32)
    if const_reward:
        return s, a, s2, np.ones((rows, 1), np.float32), np.ones((rows, 1), np.float32)
    r = rng.standard_normal((rows, 1)).astype(np.float32)
    nd = np.ones((rows, 1), np.float32)
    nd[49::50] = 0
    return s, a, s2, r, nd


def draw(rng_index, seed, call, bs, size):
    """Rows of FQE's `call`-th step (1-based): the ring gather's draw at seed + SEED_FQE_INDEX.  rng_index: the CPU twin of the device
    generator's index draw, (seed, stream, call, n, bound) -> int64[n]."""
    return np.asarray(rng_index((seed + SEED_FQE_INDEX) & 0xFFFFFFFF, GATHER_STREAM, call, bs, size), np.int64)
