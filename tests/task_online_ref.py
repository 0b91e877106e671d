"""fp64 / integer NumPy restatement of ONE interaction of the online modes (mobody_task_interact) on top of
tests/task_ref.py: both action forms, the step, the stored flag, episode end, reset, ring slots, commit and the per-lane statistics.
Shared by the CPU tests (this file against a plain per-lane loop) and the GPU tests (csrc/task_online.hip against it; the bookkeeping
of their composition is bookkeep() / record() / commit() on fp32 arrays, whose sums NumPy rounds as the device does).  Also holds
the cases of the GPU tests, so the CPU suite can check their seeds."""
import numpy as np

import bosa_graph_cases as GC
import task_ref as R
from oracle import mobody_oracle as O

STREAM_NOISE, STREAM_START, STREAM_POLICY, STREAM_EXPLORE = 4, 6, 11, 12


def action(p, head, pol, expl, n1=None, n2=None, dtype=np.float64):
    """The action of an interaction.  head 0: base = pol [lanes, A] (pi(s)); head 1: pol = mu | logstd [lanes, 2 A] and
    base = max_action tanh(mu + exp(clamp(logstd, -20, 2)) n1).  expl != 0: clamp(base + (expl max_action) n2, -max_action,
    max_action); expl == 0: base.  max_action and expl enter as the fp32 values the kernel gets."""
    A = p["A"]
    ma = dtype(np.float32(p["max_action"]))
    pol = np.asarray(pol, dtype)
    if head == 0:
        base = pol
    else:
        mu, logstd = pol[:, :A], pol[:, A:]
        base = ma * np.tanh(mu + np.exp(np.clip(logstd, -20.0, 2.0)) * np.asarray(n1, dtype))
    if float(expl) == 0.0:
        return base
    scale = dtype(np.float32(np.float32(expl) * np.float32(p["max_action"])))
    return np.clip(base + scale * np.asarray(n2, dtype), -ma, ma)


def new_lanes(start, dtype=np.float64):
    """The lanes' state and counters before the first interaction; `start` [lanes, S] the first start states."""
    n = start.shape[0]
    z = lambda t: np.zeros(n, t)
    return dict(obs=np.array(start, dtype), t=z(np.int32), ep=z(np.int32), ret=z(dtype), done_count=z(np.int32), ret_sum=z(dtype),
                len_sum=z(np.int32), count=0)


def new_ring(cap, S, A, dtype=np.float64):
    return dict(state=np.zeros((cap, S), dtype), action=np.zeros((cap, A), dtype), next_state=np.zeros((cap, S), dtype),
                reward=np.zeros(cap, dtype), not_done=np.zeros(cap, dtype), ptr=0, size=0, cap=cap)


def bookkeep(st, reward, pred, time_limit):
    """The reference's per-step rule (train_mobody.py:684-709) on every lane: t += 1; stored done = predicate and t < time_limit; the
    episode ends when the predicate holds or t == time_limit.  Returns (done, reset); the sums keep st's dtype."""
    pred = np.asarray(pred, bool)
    t_ep = st["t"] + 1
    done = pred & (t_ep < time_limit)
    reset = pred | (t_ep >= time_limit)
    ret = (st["ret"] + np.asarray(reward, st["ret"].dtype)).astype(st["ret"].dtype)
    st["done_count"] = st["done_count"] + reset
    st["ret_sum"] = np.where(reset, (st["ret_sum"] + ret).astype(ret.dtype), st["ret_sum"])
    st["len_sum"] = st["len_sum"] + np.where(reset, t_ep, 0).astype(np.int32)
    st["t"] = np.where(reset, 0, t_ep).astype(np.int32)
    st["ret"] = np.where(reset, 0, ret).astype(ret.dtype)
    st["ep"] = st["ep"] + reset
    return done, reset


def record(ring, s, a, nxt, reward, done):
    """Lane b's transition goes to row (ptr + b) mod cap; not_done = 1 - done."""
    rows = (ring["ptr"] + np.arange(s.shape[0])) % ring["cap"]
    ring["state"][rows], ring["action"][rows], ring["next_state"][rows] = s, a, nxt
    ring["reward"][rows], ring["not_done"][rows] = reward, 1.0 - np.asarray(done, ring["not_done"].dtype)
    return rows


def commit(ring, lanes):
    ring["ptr"] = (ring["ptr"] + lanes) % ring["cap"]
    ring["size"] = min(ring["size"] + lanes, ring["cap"])


def pick_start(start_fn, ep, lanes):
    """Row b of start_fn(ep[b]) for every lane ([lanes, S]): the e-th start state of lane b."""
    tables = {int(e): start_fn(int(e)) for e in np.unique(ep)}
    return np.stack([tables[int(ep[b])][b] for b in range(lanes)])


def interact(p, st, ring, head, policy_fn, time_limit, expl, normal_fn, start_fn, call0=0):
    """One interaction in fp64.  policy_fn(s) -> pi or mu | logstd; normal_fn(stream, call, n) -> n unit normals; start_fn(e) ->
    [lanes, S] start states of episode index e.  Returns the step's dict plus action, done, reset and the ring rows."""
    S, A, lanes, c = p["S"], p["A"], st["obs"].shape[0], st["count"]
    s = st["obs"].copy()
    pol = policy_fn(s)
    n1 = normal_fn(STREAM_POLICY, c, lanes * A).reshape(lanes, A) if head == 1 else None
    n2 = normal_fn(STREAM_EXPLORE, c, lanes * A).reshape(lanes, A) if float(expl) != 0.0 else None
    a = action(p, head, pol, expl, n1, n2)
    r = R.step(p, s, a, normal_fn(STREAM_NOISE, call0 + c, lanes * S).reshape(lanes, S))
    done, reset = bookkeep(st, r["reward"], r["terminal"], time_limit)
    rows = record(ring, s, a, r["next"], r["reward"], done)
    commit(ring, lanes)
    st["obs"] = np.where(reset[:, None], pick_start(start_fn, st["ep"], lanes), r["next"])
    st["count"] = c + 1
    return dict(r, action=a, done=done, reset=reset, rows=rows)


def episode_stats(st):
    """OnlineTask.episode_stats: the per-lane accumulators added in lane order, then cleared."""
    n = int(st["done_count"].sum())
    out = dict(episodes=n, return_mean=None, length_mean=None)
    if n:
        out.update(return_mean=float(np.sum(st["ret_sum"].astype(np.float64))) / n, length_mean=float(st["len_sum"].sum()) / n)
    for k in ("done_count", "ret_sum", "len_sum"):
        st[k] = np.zeros_like(st[k])
    return out


# ---- the cases of the GPU tests (tests/test_hip_task_online.py) ---------------------------------------------------------------------
SEED, CALL0, TIME_LIMIT, INTERACTIONS = 20262, 3, 5, 24
SHAPES = [(3, 1, "hopper-medium-v2"), (11, 3, "hopper-medium-v2"), (17, 6, "walker2d-medium-v2"), (111, 8, "ant-medium-v2")]


def lane_counts(S):
    """Lane counts around the workgroup's 256 / S lanes: a ragged workgroup, exactly one, one more (0 is skipped where it arises)."""
    rpb = 256 // S
    return sorted({n for n in (1, rpb - 1, rpb, rpb + 1) if n >= 1})


def ring_cap(lanes):
    """A ring that is no multiple of the lane count (except at one lane) and wraps within a few interactions."""
    return 3 * lanes + 1


def case_params(S, A, task):
    """A shifted domain with exact fp32 values; the walker and ant shapes with a stronger pull so that lanes fall within the run."""
    return R.params(S, A, task, f=1.5, grav=4.0, gain=[0.5] + [0.75] * (A - 1))


def philox_normal(seed):
    return lambda stream, call, n: O.rng_normal(seed, stream, call, n).astype(np.float64)


def case_init_std(task):
    """Start states wide enough that some lanes leave the alive set within the run: the hopper's |angle| < 0.2 is near, the walker's
    and the ant's height bands are 0.4 away."""
    return 0.12 if "hopper" in task else 0.3


def case_start(p, lanes, seed):
    mu, init_std = R.f32(p["mu"]), case_init_std(p["task"])
    return lambda e: mu + float(np.float32(init_std)) * O.rng_normal(seed, STREAM_START, e, lanes * p["S"]).reshape(lanes, p["S"]).astype(np.float64)


def case_policy(S, A, head, seed=5):
    """fp64 forward of the packed_policy net of the GPU tests (tests/test_hip_fqe.py: GC.mlp_params(seed, S, out, 1)); head 0 with
    the tanh of out_mode 1."""
    params = GC.mlp_params(seed, S, A if head == 0 else 2 * A, 1)[0]
    if head == 0:
        return lambda s: np.tanh(GC.mlp(params, s, np.float64))
    return lambda s: GC.mlp(params, s, np.float64)


def run_case(S, A, task, lanes, head, expl, interactions=INTERACTIONS):
    """The GPU case rolled through the restatement: (per-interaction results, lanes' state, ring)."""
    p = case_params(S, A, task)
    start = case_start(p, lanes, SEED)
    st, ring = new_lanes(start(0)), new_ring(ring_cap(lanes), S, A)
    pol, normal = case_policy(S, A, head), philox_normal(SEED)
    out = [interact(p, st, ring, head, pol, TIME_LIMIT, expl, normal, start, call0=CALL0) for _ in range(interactions)]
    return p, out, st, ring
