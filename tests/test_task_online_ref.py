"""The restatement of one online interaction (tests/task_online_ref.py) on its own: against a plain per-lane loop written the way the
reference's mode-1 loop is (train_mobody.py:677-709), the two action forms term by term, the seeds of the GPU cases against the
termination thresholds, and the stream ids / binding of the new entry point.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import task_online_ref as OR
import task_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def numpy_normal(seed):
    """Unit normals keyed by (stream, call): the same draw whoever asks, as the device generator gives."""
    return lambda stream, call, n: np.random.default_rng([seed, stream, call]).standard_normal(n)


def plain_loop(p, lanes, cap, time_limit, interactions, head, expl, policy_fn, normal_fn, start_fn, call0):
    """`lanes` environments driven one after the other, each the way the reference drives its one (train_mobody.py:677-709): count
    the step, select the action, step, done_bool = done if timesteps < max_episode_steps else 0, ReplayBuffer.add, and on done log
    the episode and reset.  `done` is gym's: the predicate, or the TimeLimit wrapper's cut."""
    S, A = p["S"], p["A"]
    ma = float(np.float32(p["max_action"]))
    buf = dict(state=np.zeros((cap, S)), action=np.zeros((cap, A)), next_state=np.zeros((cap, S)), reward=np.zeros(cap),
               not_done=np.zeros(cap), ptr=0, size=0)
    state = [start_fn(0)[b] for b in range(lanes)]
    episode_reward, episode_timesteps, episode_num = [0.0] * lanes, [0] * lanes, [0] * lanes
    logged, kinds = [[] for _ in range(lanes)], dict(wrap=0, limit=0, predicate=0)
    for t in range(interactions):
        n1 = normal_fn(OR.STREAM_POLICY, t, lanes * A).reshape(lanes, A)
        n2 = normal_fn(OR.STREAM_EXPLORE, t, lanes * A).reshape(lanes, A)
        ns = normal_fn(OR.STREAM_NOISE, call0 + t, lanes * S).reshape(lanes, S)
        for b in range(lanes):
            episode_timesteps[b] += 1
            out = policy_fn(state[b][None])[0]
            if head == 0:
                act = [float(x) for x in out]
            else:                                            # iql.py:74-89: rsample of the tanh-transformed normal, times max_action
                act = [ma * math.tanh(float(out[j]) + math.exp(min(max(float(out[A + j]), -20.0), 2.0)) * float(n1[b, j])) for j in range(A)]
            if expl != 0.0:                                  # train_mobody.py:733-735
                sd = float(np.float32(np.float32(expl) * np.float32(p["max_action"])))
                act = [min(max(x + sd * float(n2[b, j]), -ma), ma) for j, x in enumerate(act)]
            r = R.step(p, state[b][None], np.array(act)[None], ns[b][None])
            next_state, reward, pred = r["next"][0], float(r["reward"][0]), bool(r["terminal"][0])
            done = pred or episode_timesteps[b] >= time_limit
            done_bool = float(done) if episode_timesteps[b] < time_limit else 0
            i = buf["ptr"]                                   # ReplayBuffer.add, utils.py:25-41
            buf["state"][i], buf["action"][i], buf["next_state"][i] = state[b], act, next_state
            buf["reward"][i], buf["not_done"][i] = reward, 1.0 - done_bool
            kinds["wrap"] += int(i + 1 == cap)
            buf["ptr"], buf["size"] = (i + 1) % cap, min(buf["size"] + 1, cap)
            state[b] = next_state
            episode_reward[b] += reward
            if done:
                kinds["predicate" if pred else "limit"] += 1
                logged[b].append((episode_reward[b], episode_timesteps[b]))
                episode_num[b] += 1
                state[b] = start_fn(episode_num[b])[b]
                episode_reward[b], episode_timesteps[b] = 0.0, 0
    return buf, np.array(state), episode_reward, episode_timesteps, episode_num, logged, kinds


@pytest.mark.parametrize("head,expl", [(0, 0.2), (1, 0.0), (0, 0.0), (1, 0.2)])
def test_interaction_equals_the_per_lane_loop(head, expl):
    S, A, lanes, limit, cap, n = 11, 3, 3, 7, 10, 40
    p = R.params(S, A, "hopper-medium-v2", f=1.5, grav=4.0, gain=[0.5, 0.75, 0.75])
    mu = R.f32(p["mu"])
    start = lambda e: mu + 0.12 * np.random.default_rng([9, e]).standard_normal((lanes, S))
    normal, pol = numpy_normal(4), OR.case_policy(S, A, head)
    if head == 1:                                            # log-stds on both sides of the clamp [-20, 2]
        inner = pol
        pol = lambda s: inner(s) * np.concatenate([np.ones(A), [60.0, -300.0, 1.0]])
    st, ring = OR.new_lanes(start(0)), OR.new_ring(cap, S, A)
    stats = []
    for k in range(n):
        OR.interact(p, st, ring, head, pol, limit, expl, normal, start, call0=100)
        if k % 13 == 12:
            stats.append(OR.episode_stats(st))
    stats.append(OR.episode_stats(st))
    buf, state, ep_rew, ep_t, ep_num, logged, kinds = plain_loop(p, lanes, cap, limit, n, head, expl, pol, normal, start, 100)
    assert kinds["wrap"] >= 1 and kinds["limit"] >= 1 and kinds["predicate"] >= 1, kinds
    for k in ("state", "action", "next_state", "reward"):
        np.testing.assert_allclose(ring[k], buf[k], rtol=0, atol=1e-12, err_msg=k)
    assert np.array_equal(ring["not_done"], buf["not_done"]) and (ring["ptr"], ring["size"]) == (buf["ptr"], buf["size"]) == (n * lanes % cap, cap)
    assert set(np.unique(ring["not_done"])) <= {0.0, 1.0}
    np.testing.assert_allclose(st["obs"], state, rtol=0, atol=1e-12)
    np.testing.assert_allclose(st["ret"], ep_rew, rtol=0, atol=1e-12)
    assert st["t"].tolist() == ep_t and st["ep"].tolist() == ep_num and st["count"] == n
    episodes = [e for lane in logged for e in lane]
    assert sum(s["episodes"] for s in stats) == len(episodes)
    total = sum(s["return_mean"] * s["episodes"] for s in stats if s["episodes"])
    assert total == pytest.approx(sum(e[0] for e in episodes), abs=1e-9)
    assert sum(s["length_mean"] * s["episodes"] for s in stats if s["episodes"]) == pytest.approx(sum(e[1] for e in episodes))
    assert OR.episode_stats(st) == dict(episodes=0, return_mean=None, length_mean=None)          # cleared by the read
    # a time-limit end stores done = 0, a predicate end before the limit done = 1 (both kinds are in the ring's last rows or were)
    assert all(length <= limit for _, length in episodes) and any(length == limit for _, length in episodes)


def test_action_forms_term_by_term():
    p = R.params(11, 3, "hopper-medium-v2", max_action=1.5)
    rng = np.random.default_rng(0)
    pi, n1, n2 = rng.uniform(-1.5, 1.5, (4, 3)), rng.standard_normal((4, 3)), rng.standard_normal((4, 3))
    assert np.array_equal(OR.action(p, 0, pi, 0.0), pi)                                         # nothing drawn, a = base
    got = OR.action(p, 0, pi, 0.2, None, n2)
    sd = float(np.float32(np.float32(0.2) * np.float32(1.5)))
    assert np.array_equal(got, np.clip(pi + sd * n2, -1.5, 1.5)) and (np.abs(got) == 1.5).any()
    pol = np.concatenate([rng.standard_normal((4, 3)), np.array([[-25.0, 0.0, 3.0]] * 4)], 1)
    got = OR.action(p, 1, pol, 0.0, n1)
    std = np.array([math.exp(-20.0), 1.0, math.exp(2.0)])
    np.testing.assert_allclose(got, 1.5 * np.tanh(pol[:, :3] + std * n1), rtol=1e-15)
    assert (np.abs(got) <= 1.5).all()


def test_gpu_cases_keep_clear_of_the_termination_thresholds():
    """The seeds of tests/test_hip_task_online.py rolled through the restatement: at most 1 % of the rows of a shape have a predicate
    quantity within 4 one-step bounds of its threshold (DESIGN 5zf's cap), and predicate ends, time-limit ends and ring wraps all
    occur in every shape."""
    for S, A, task in OR.SHAPES:
        near = rows = pred_ends = limit_ends = 0
        for lanes in OR.lane_counts(S):
            for head, expl in ((0, 0.0), (0, 0.2), (1, 0.0)):
                p, out, st, ring = OR.run_case(S, A, task, lanes, head, expl)
                for r in out:
                    near += int(R.near_threshold(p, r).sum())
                    rows += lanes
                    pred_ends += int((r["reset"] & r["terminal"]).sum())
                    limit_ends += int((r["reset"] & ~r["terminal"]).sum())
                assert OR.INTERACTIONS * lanes > ring["cap"] and ring["size"] == ring["cap"]
        print(f"online cases S={S} A={A}: {rows} rows, {near} near a threshold, {pred_ends} predicate ends, {limit_ends} time-limit ends")
        assert near <= 0.01 * rows, (S, A, near, rows)
        assert pred_ends >= 1 and limit_ends >= 1, (S, A, pred_ends, limit_ends)


def test_stream_ids_and_binding_of_the_entry_point():
    from mobody_amd import _lib, task
    hdr = open(os.path.join(ROOT, "include", "mobody_hip.h")).read()
    ids = {k: int(v) for k, v in re.findall(r"MOBODY_TASK_STREAM_(\w+) = (\d+)", hdr)}
    assert (ids["POLICY"], ids["EXPLORE"]) == (OR.STREAM_POLICY, OR.STREAM_EXPLORE) == (task.STREAM_POLICY, task.STREAM_EXPLORE)
    taken = {int(v) for k, v in re.findall(r"(\w*STREAM\w*) = (\d+)", hdr) if "TASK_STREAM_POLICY" not in k and "TASK_STREAM_EXPLORE" not in k}
    assert not {ids["POLICY"], ids["EXPLORE"]} & (taken | {1, 2, 3} | set(range(16, 23))) and ids["POLICY"] != ids["EXPLORE"]
    assert "mobody_task_interact" in _lib.PROTOTYPES and "mobody_task_interact_workspace" in _lib.PROTOTYPES
    assert _lib.BLOCK_BYTES[_lib.MobodyTaskInteract] % 8 == 0
