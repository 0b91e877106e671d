"""One online interaction on the device (csrc/task_online.hip; mobody_amd/task.py OnlineTask): `mobody_task_interact` bit for
bit against the composition of `mobody_mlp3_forward`, `mobody_rng_normal`, torch's clamp, `mobody_task_step` and `mobody_ring_append`
with the bookkeeping of the restatement (tests/task_online_ref.py); the Gaussian head against fp64 within a derived bound; graph
replay; isolation; the refusals; and `--mode 1` / `--mode 2` of the driver end to end."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import task_online_ref as OR
import task_ref as R
from test_hip_fqe import cli_args, differing, packed_policy, snapshot
from test_hip_task import T, bits, device_params, scalars

pytestmark = pytest.mark.gpu

LANE_KEYS = ("lane_obs", "lane_t", "lane_ep", "lane_ret", "done_count", "ret_sum", "len_sum", "count")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Ring:
    """A row-interleaved ring of `cap` rows and its device words, every byte pre-filled with a pattern."""

    def __init__(self, cap, S, A, dev):
        from mobody_amd import ops
        self.cap, self.S, self.A = cap, S, A
        self.store = torch.empty(cap, ops.ring_pitch(S, A), dtype=torch.float32, device=dev)
        self.store.view(torch.uint8).fill_(0xA5)
        self.view = ops.RingView(self.store, S, A)
        self.ptr_size = torch.zeros(2, dtype=torch.int64, device=dev)


class Case:
    """One GPU case of task_online_ref: the task, a policy net, and two sides that start equal -- the fused entry point's lanes and
    ring, and the composition's (lanes on the host in fp32, ring on the device)."""

    def __init__(self, S, A, task, lanes, head, expl, dev, mfma, net=None):
        from mobody_amd import ops
        self.S, self.A, self.lanes, self.head, self.expl, self.dev = S, A, lanes, head, float(expl), dev
        self.p = OR.case_params(S, A, task)
        self.dp = device_params(self.p, dev)
        self.net = net if net is not None else packed_policy(S, A, head, dev, mfma)[0]
        self.init_std = OR.case_init_std(task)
        self.mu = T(self.p["mu"], dev)
        cap = OR.ring_cap(lanes)
        self.fused_ring, self.comp_ring = Ring(cap, S, A, dev), Ring(cap, S, A, dev)
        start = self.start(0)
        self.state = ops.online_state(lanes, S, dev)
        self.state["lane_obs"].copy_(start)
        self.st = OR.new_lanes(start.cpu().numpy(), np.float32)
        self.ws = None

    def start(self, e):
        from mobody_amd import ops
        eps = ops.rng_normal(OR.SEED, OR.STREAM_START, e, self.lanes * self.S, self.dev).reshape(self.lanes, self.S)
        return self.mu + np.float32(self.init_std) * eps

    def fused(self):
        from mobody_amd import ops
        r = self.fused_ring
        self.ws = ops.task_interact(self.dp, self.net.blob, self.head, r.view, r.cap, r.ptr_size, self.state, OR.TIME_LIMIT, self.expl,
                                    self.init_std, OR.SEED, call0=OR.CALL0, ws=self.ws, policy_blob_T=self.net.blob_T,
                                    precision=self.net.precision)

    def forward(self, obs):
        from mobody_amd import ops
        n = self.net
        return ops.mlp3_forward(n.blob, self.S, n.out_dim, 1, obs, out_mode=1 if self.head == 0 else 0, max_action=self.p["max_action"],
                                blob_T=n.blob_T, precision=n.precision)[0]

    def head0_action(self, obs):
        """pi(s) and, with expl != 0, the clamp formed in torch in the written operation order."""
        from mobody_amd import ops
        base = self.forward(obs)
        if self.expl == 0.0:
            return base
        ma = float(np.float32(self.p["max_action"]))
        scale = float(np.float32(np.float32(self.expl) * np.float32(ma)))
        n2 = ops.rng_normal(OR.SEED, OR.STREAM_EXPLORE, self.st["count"], self.lanes * self.A, self.dev).reshape(self.lanes, self.A)
        return torch.clamp(base + scale * n2, -ma, ma)

    def compose(self, act):
        """The rest of the interaction from the existing entry points, fed the action `act`; bookkeeping from the restatement."""
        from mobody_amd import ops
        st, r = self.st, self.comp_ring
        obs = T(st["obs"], self.dev)
        out = ops.task_step(self.dp, obs, act.contiguous(), seed=OR.SEED, call=OR.CALL0 + st["count"])
        reward, pred = out["reward"].cpu().numpy(), out["terminal"].cpu().numpy() != 0
        done, reset = OR.bookkeep(st, reward, pred, OR.TIME_LIMIT)
        ops.ring_append(r.view, r.cap, r.ptr_size, self.S, self.A, obs, act.contiguous(), out["next_obs"], out["reward"],
                        T(done.astype(np.uint8), self.dev))
        nxt = out["next_obs"].cpu().numpy()
        if reset.any():
            fresh = OR.pick_start(lambda e: self.start(e).cpu().numpy(), st["ep"], self.lanes)
            nxt = np.where(reset[:, None], fresh, nxt)
        st["obs"] = nxt.astype(np.float32)
        st["count"] += 1
        return pred, reset

    def assert_equal(self, where):
        st, got = self.st, {k: v.cpu().numpy() for k, v in self.state.items()}
        want = dict(lane_obs=st["obs"], lane_t=st["t"], lane_ep=st["ep"], lane_ret=st["ret"], done_count=st["done_count"],
                    ret_sum=st["ret_sum"], len_sum=st["len_sum"], count=np.array([st["count"]], np.int64))
        for k in LANE_KEYS:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (where, k)
        assert torch.equal(self.fused_ring.ptr_size, self.comp_ring.ptr_size), (where, self.fused_ring.ptr_size, self.comp_ring.ptr_size)
        assert torch.equal(bits(self.fused_ring.store), bits(self.comp_ring.store)), (where, "ring storage")


# ---- 1. equal to the composition, bit for bit (head 0) ------------------------------------------------------------------------------
@pytest.mark.parametrize("S,A,task", OR.SHAPES, ids=[f"S{s[0]}A{s[1]}" for s in OR.SHAPES])
def test_interaction_equals_the_composition_bit_for_bit(S, A, task, mfma, dev):
    ends = dict(pred=0, limit=0)
    for lanes in OR.lane_counts(S):
        for expl in (0.0, 0.2):
            c = Case(S, A, task, lanes, 0, expl, dev, mfma)
            for k in range(OR.INTERACTIONS):
                act = c.head0_action(T(c.st["obs"], dev))
                c.fused()
                pred, reset = c.compose(act)
                ends["pred"] += int((reset & pred).sum())
                ends["limit"] += int((reset & ~pred).sum())
                c.assert_equal((S, A, lanes, expl, k))
            assert int(c.fused_ring.ptr_size[1]) == c.fused_ring.cap and c.st["count"] * lanes > c.fused_ring.cap      # wrapped
            if expl:
                a = c.fused_ring.view[1]
                assert float(a.abs().max()) <= 1.0 and not torch.equal(a, c.forward(c.fused_ring.view[0].contiguous()))    # the noise is in
    assert ends["pred"] >= 1 and ends["limit"] >= 1, ends


# ---- 2. the Gaussian head ------------------------------------------------------------------------------------------------------------
# a = max_action * tanhf(mu + expf(clamp(logstd)) * n1) against the fp64 value formed from the same fp32 mu, logstd and n1.  With
# u = 2^-24 (half an ulp): the device expf is within 1 ulp (relative 2 u), the product std * n rounds once (u) and the sum once (u of
# |mu| + std |n|): the argument of tanh is off by at most 2 u std |n| + u std |n| + u (|mu| + std |n|) <= 4 u (|mu| + std |n|); tanh is
# 1-Lipschitz, so that is also the error it hands on; the device tanhf is within 2 ulp of a value of at most 1 (4 u), and the product
# with max_action rounds once (u).  Sum: max_action u (5 + 4 (|mu| + std |n|)) <= 6 u max_action (1 + |mu| + std |n|), the last unit of
# the constant covering the second-order terms.
HEAD1_C = 6.0


def gaussian_net(S, A, dev, mfma):
    """The test policy with log-std biases on both sides of the clamp [-20, 2] and inside it."""
    net, params = packed_policy(S, A, 1, dev, mfma)
    import bosa_graph_cases as GC
    p = [x.copy() for x in params[0]]
    p[5][A:] += np.resize(np.array([30.0, -40.0, 0.5, -3.0], np.float32), A)
    net.load_state_dict({k: torch.from_numpy(v).to(dev) for k, v in GC.state_dict([p], ("",)).items()})
    return net


@pytest.mark.parametrize("S,A,task", OR.SHAPES, ids=[f"S{s[0]}A{s[1]}" for s in OR.SHAPES])
def test_gaussian_head_within_the_derived_bound_and_downstream_bits(S, A, task, mfma, dev):
    from mobody_amd import ops
    worst, outside = 0.0, 0
    for lanes in OR.lane_counts(S)[-2:]:
        c = Case(S, A, task, lanes, 1, 0.0, dev, mfma, net=gaussian_net(S, A, dev, mfma))
        for k in range(12):
            obs = T(c.st["obs"], dev)
            raw = c.forward(obs).cpu().numpy().astype(np.float64)
            n1 = ops.rng_normal(OR.SEED, OR.STREAM_POLICY, c.st["count"], lanes * A, dev).reshape(lanes, A).cpu().numpy().astype(np.float64)
            rows = (int(c.fused_ring.ptr_size[0]) + np.arange(lanes)) % c.fused_ring.cap
            c.fused()
            act = c.fused_ring.view[1][torch.as_tensor(rows, device=dev)].contiguous()
            want = OR.action(c.p, 1, raw, 0.0, n1)
            mu, logstd = raw[:, :A], raw[:, A:]
            std = np.exp(np.clip(logstd, -20.0, 2.0))
            bound = HEAD1_C * 2.0 ** -24 * c.p["max_action"] * (1.0 + np.abs(mu) + std * np.abs(n1))
            err = np.abs(act.cpu().numpy().astype(np.float64) - want)
            worst = max(worst, float((err / bound).max()))
            outside += int(((logstd < -20.0) | (logstd > 2.0)).sum())
            assert (err <= bound).all(), (S, A, lanes, k, float((err / bound).max()))
            c.compose(act)                                   # everything downstream: bit-equal when fed the RECORDED action
            c.assert_equal((S, A, lanes, k))
    print(f"task_interact head 1 S={S} A={A} {mfma}: worst error / bound {worst:.4f} (c = {HEAD1_C:g}), {outside} log-stds outside [-20, 2]")
    assert outside >= 1


# ---- 3 / 4. OnlineTask: graph replay, isolation, the host cache -----------------------------------------------------------------------
def online_pair(dev, mfma, head, expl, rng):
    from mobody_amd.algo import utils
    from mobody_amd.task import Task, TaskSpec
    task = Task(TaskSpec.from_env("hopper-friction", "2.0", "target"), dev, seed=3)
    buf = utils.ReplayBuffer(11, 3, dev, max_size=16, rng="device", seed=9)
    buf.store.view(torch.uint8).fill_(0xA5)
    return task, buf, task.online(buf, lanes=5, time_limit=4, expl=expl, rng=rng), packed_policy(11, 3, head, dev, mfma)[0]


@pytest.mark.parametrize("head,expl", [(0, 0.2), (1, 0.0)])
def test_replayed_interaction_has_the_bits_of_the_eager_one(head, expl, mfma, dev):
    _, buf_e, eager, net = online_pair(dev, mfma, head, expl, "numpy")
    _, buf_g, graph, _ = online_pair(dev, mfma, head, expl, "device")
    for k in range(30):
        eager.interact(net, head)
        graph.interact(net, head)
    torch.cuda.synchronize()
    assert graph.captures == 1 and eager.captures == 0
    assert torch.equal(bits(buf_e.store), bits(buf_g.store)) and torch.equal(buf_e.ptr_size, buf_g.ptr_size)
    for k in LANE_KEYS:
        assert torch.equal(bits(eager.state[k]), bits(graph.state[k])), k
    assert int(graph.state["count"]) == 30 and int(graph.state["lane_ep"].min()) >= 7          # resets (time_limit 4) and wraps (16 rows)
    se, sg = eager.episode_stats(), graph.episode_stats()
    assert se == sg and se["episodes"] >= 35 and se["length_mean"] <= 4.0
    assert graph.episode_stats()["episodes"] == 0


def test_interact_moves_no_generator_no_draw_count_and_keeps_the_host_cache(mfma, dev):
    task, buf, online, net = online_pair(dev, mfma, 1, 0.2, "device")
    before = (torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()[1].copy(), buf._draws, snapshot(task))
    pulls = []
    buf._pull = lambda: pulls.append(1)
    for k in range(30):
        online.interact(net, 1)
    torch.cuda.synchronize()
    assert torch.equal(before[0], torch.get_rng_state()) and torch.equal(before[1], torch.cuda.get_rng_state())
    assert np.array_equal(before[2], np.random.get_state()[1]) and buf._draws == before[3] and pulls == []
    assert differing(before[4], snapshot(task)) == []
    assert [buf.ptr, buf.size] == buf.ptr_size.tolist() == [30 * 5 % 16, 16] and online.interactions == 30


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field_and_touch_nothing(dev):
    from mobody_amd import _lib, ops
    lib = ops.load()
    S, A, lanes = 11, 3, 4
    p = OR.case_params(S, A, "hopper-medium-v2")
    ring = Ring(8, S, A, dev)
    state = ops.online_state(lanes, S, dev)
    # (a real net and real sizes behind every pointer: a refusal that failed to refuse would still launch in bounds)
    extra = dict(blob=packed_policy(S, A, 0, dev)[0].blob, ws=torch.empty(256, device=dev))
    for v in list(state.values()) + [extra["ws"]]:
        v.view(torch.uint8).fill_(0xA5)
    before = {k: v.clone() for k, v in dict(state, store=ring.store, ptr_size=ring.ptr_size, **extra).items()}
    view = ops.buffer_view(ring.view)

    def params(**over):
        dp = device_params(p, dev)
        for k, v in over.items():
            setattr(dp, k, v)
        return dp

    def blk(dp=None, ring_view=view, **f):
        base = dict(policy_blob=extra["blob"].data_ptr(), lanes=lanes, cap=8, head=0, time_limit=5, expl=0.0, init_std=0.1, seed=1,
                    ring=C.pointer(ring_view) if ring_view is not None else None, ptr_size=ring.ptr_size.data_ptr(),
                    workspace=extra["ws"].data_ptr(), **{k: v.data_ptr() for k, v in state.items()})
        return _lib.block(_lib.MobodyTaskInteract, p=dp or params(), **dict(base, **f))

    def refused(b, *words):
        assert lib.mobody_task_interact(C.byref(b), None) == -1
        msg = lib.mobody_last_error().decode()
        assert msg.startswith("mobody_task_interact:") or msg.startswith("mobody_mlp_layout:"), msg
        for w in words:
            assert w in msg, (w, msg)

    refused(_lib.MobodyTaskInteract(struct_bytes=C.sizeof(_lib.MobodyTaskInteract) - 8), "struct_bytes")
    refused(blk(params(S=2)), "S 2")
    refused(blk(params(S=257)), "S 257")
    refused(blk(params(A=0)), "A 0")
    refused(blk(params(A=65)), "A 65")
    refused(blk(params(task=9)), "task")
    refused(blk(params(task=6)), "pen")
    refused(blk(params(max_action=0.0)), "max_action")
    for f in ("mu", "gain", "bmat"):
        refused(blk(params(**{f: None})), "null pointer " + f)
    refused(blk(head=2), "head 2")
    refused(blk(head=-1), "head -1")
    refused(blk(lanes=-1), "lanes < 0")
    refused(blk(lanes=9), "lanes 9 > cap 8")
    refused(blk(time_limit=0), "time_limit")
    refused(blk(expl=-0.1), "expl")
    refused(blk(expl=float("nan")), "expl")
    refused(blk(precision=7), "precision")
    refused(blk(precision=4), "T blob")
    for f in ("policy_blob", "ring", "ptr_size", "workspace") + LANE_KEYS:
        refused(blk(**{f: None}), "null pointer " + f)
    hole = ops.buffer_view(ring.view)
    hole.reward = None
    refused(blk(ring_view=hole), "null pointer", "ring")
    assert lib.mobody_task_interact(C.byref(blk(lanes=0)), None) == 0                       # lanes == 0: nothing is written
    assert lib.mobody_task_interact_workspace(C.byref(_lib.MobodyTaskInteract(struct_bytes=8))) == -1
    assert lib.mobody_task_interact_workspace(C.byref(blk(head=1))) == (2 * lanes * A + 3) // 4 * 4
    torch.cuda.synchronize()
    for k, v in dict(state, store=ring.store, ptr_size=ring.ptr_size, **extra).items():
        assert torch.equal(bits(v), bits(before[k])), k


# ---- 6. the driver ---------------------------------------------------------------------------------------------------------------------
def online_cli(tmp_path, policy, mode, steps, eval_freq, **params):
    return ["--policy", policy, "--env", "hopper-friction", "--shift_level", "2.0", "--mode", str(mode), "--seed", "1", "--synthetic", "2",
            "--tartype", "medium", "--srctype", "expert", "--rng", "device", "--src_rows", "4000", "--tar_rows", "4000",
            "--tar_env_interact_interval", "10", "--max_step", str(steps), "--eval_freq", str(eval_freq), "--log_every", str(max(steps, 1)),
            "--dir", str(tmp_path), "--params", json.dumps(dict(dict(batch_size=64, graph=1, task_eval_episodes=8, task_episode_steps=25), **params))]


def run_driver(monkeypatch, argv):
    from mobody_amd import train_mobody as tm
    from mobody_amd.algo import utils
    made = []
    init = utils.ReplayBuffer.__init__
    monkeypatch.setattr(utils.ReplayBuffer, "__init__", lambda self, *a, **k: (init(self, *a, **k), made.append(self))[0])
    pol = tm.main(argv)
    torch.cuda.synchronize()
    monkeypatch.setattr(utils.ReplayBuffer, "__init__", init)
    return pol, made[-2], made[-1]                           # the driver's two, built after whatever the policy builds for itself


def check_rows(rb, n, lanes, domain, seed, dev, limit=25):
    """Rows [0, n) of an online buffer: each a valid transition of the `domain` task under the restatement given its recorded (s, a)
    and the process noise of its interaction, to DESIGN 5zf's one-step bound; lane b's rows chain (state = the row before's next state
    unless an episode ended there).  Returns the finished episodes [(row of the last step, return, length)]."""
    from mobody_amd import ops
    from mobody_amd.task import SEED_TASK_ONLINE
    p = R.from_env("hopper-friction", "2.0", domain)
    S, A = p["S"], p["A"]
    assert rb.size == n and rb.ptr == n % rb.max_size and rb.ptr_size.tolist() == [n % rb.max_size, n]
    s, a, s2, r, nd = (t[:n].cpu().numpy().astype(np.float64) for t in rb.sample_all())
    assert float(rb.store[n:n + 64].abs().max()) == 0.0                                       # nothing behind the rows
    noise = np.concatenate([ops.rng_normal((seed + SEED_TASK_ONLINE) & 0xFFFFFFFF, OR.STREAM_NOISE, 1 + k, lanes * S, dev).reshape(lanes, S).cpu().numpy()
                            for k in range(n // lanes)]).astype(np.float64)
    want = R.step(p, s, a, noise)
    e_n, e_r = np.abs(s2 - want["next"]) / R.bound(p, want["mag_next"]), np.abs(r[:, 0] - want["reward"]) / R.bound(p, want["mag_reward"])
    print(f"online rows ({domain}): next err/bound {float(e_n.max()):.4f}, reward {float(e_r.max()):.4f}")
    assert (e_n <= 1.0).all() and (e_r <= 1.0).all()
    near = R.near_threshold(p, want)
    assert near.sum() <= 0.01 * n
    episodes = []
    for b in range(lanes):
        t, ret = 0, 0.0
        for i in range(b, n, lanes):
            t, ret = t + 1, ret + r[i, 0]
            ended = bool(want["terminal"][i]) or t == limit
            if not near[i]:
                assert nd[i, 0] == (0.0 if want["terminal"][i] and t < limit else 1.0), i
            if i + lanes < n:
                assert np.array_equal(s[i + lanes], s2[i]) != ended or near[i], i
            if ended:
                episodes.append((i, ret, t))
                t, ret = 0, 0.0
    return episodes


def test_cli_mode1_fills_the_target_buffer_from_the_target_task(tmp_path, monkeypatch, dev):
    pol, src_rb, tar_rb = run_driver(monkeypatch, online_cli(tmp_path, "TD3_BC", 1, 600, 200, online_lanes=2))
    assert src_rb.size == 4000
    episodes = check_rows(tar_rb, 120, 2, "target", 1 + 2, dev)
    rows = scalars(tmp_path)
    logged = {s: v for t, s, v in rows if t == "train/target return"}
    counts = {s: v for t, s, v in rows if t == "train/episodes"}
    assert episodes and logged and not any(t == "train/source return" for t, _, _ in rows)
    prev = 0
    for step in (200, 400, 600):                             # interaction k runs before train step 10 k: rows 2 k, 2 k + 1
        mine = [e for e in episodes if prev <= e[0] // 2 * 10 < step]
        prev = step
        if mine:
            assert counts[step] == len(mine) and logged[step] == pytest.approx(np.mean([e[1] for e in mine]), rel=1e-5)
        else:
            assert step not in logged
    final = [v for t, s, v in rows if t == "test/target return" and s == 600]
    assert len(final) == 1 and np.isfinite(final[0]) and all(np.isfinite(v) for _, _, v in rows)
    assert not any(t == "data/target return" for t, _, _ in rows) and any(t == "data/source return" for t, _, _ in rows)


def test_cli_mode2_fills_the_source_buffer_with_sampled_noisy_actions(tmp_path, monkeypatch, dev):
    from mobody_amd import ops, task
    means, interact = [], task.OnlineTask.interact

    def spy(self, net, head):                                # max_action tanh(mu) of the acting policy, as it is at this interaction
        means.append(ops.mlp3_forward(net.blob, 11, 6, 1, self.state["lane_obs"], out_mode=1, max_action=1.0, blob_T=net.blob_T,
                                      precision=net.precision)[0][:, :3].clone())
        assert head == 1
        return interact(self, net, head)

    monkeypatch.setattr(task.OnlineTask, "interact", spy)
    pol, src_rb, tar_rb = run_driver(monkeypatch, online_cli(tmp_path, "IQL", 2, 200, 100))
    assert tar_rb.size == 4000 and len(means) == 200
    check_rows(src_rb, 200, 1, "source", 1 + 1, dev)
    a = src_rb.action[:200]
    off = (a - torch.cat(means)).abs().max(dim=1).values          # the sample and the exploration noise are in
    assert int((off > 1e-3).sum()) >= 190 and float(a.abs().max()) <= 1.0 and len(torch.unique(a)) > 300
    tags = {t for t, _, _ in scalars(tmp_path)}
    assert "train/source return" in tags and "train/episodes" in tags and "train/target return" not in tags


def test_cli_refusals_exit_with_their_reason(tmp_path, monkeypatch):
    from mobody_amd import train_mobody as tm
    from test_hip_bosa_class import config_tree

    def refused(argv, match):
        with pytest.raises(SystemExit, match=match):
            tm.main(argv)

    def swap(argv, flag, value):
        argv = list(argv)
        argv[argv.index(flag) + 1] = value
        return argv

    good = online_cli(tmp_path, "TD3_BC", 1, 4, 2)
    refused(swap(good, "--synthetic", "1"), "--synthetic 2")
    refused(swap(swap(good, "--mode", "2"), "--synthetic", "1"), "--synthetic 2")
    refused(swap(good, "--policy", "MOBODY"), "mode-3 branch")
    refused(swap(good, "--mode", "0"), "SAC is not in the reference tree")
    for key in ("model_eval_episodes", "model_error_horizon", "fqe_steps"):
        refused(online_cli(tmp_path, "TD3_BC", 1, 4, 2, **{key: 4}), key)
    monkeypatch.setenv("MOBODY_CONFIG_ROOT", config_tree(tmp_path, vae_iteration=5, batch_size=8))
    refused(swap(swap(good, "--policy", "BOSA"), "--env", "walker2d-friction"), "critic_actor")      # (the tree holds walker2d's file)
    monkeypatch.setenv("WORLD_SIZE", "2")
    refused(good, "more than one rank")


def test_cli_mode3_given_or_omitted_is_one_run(tmp_path, monkeypatch):
    from mobody_amd import train_mobody as tm
    argv, params = cli_args("IQL", tmp_path, monkeypatch)
    runs = {}
    for key in ("given", "omitted"):
        av = list(argv)
        if key == "omitted":
            i = av.index("--mode")
            del av[i:i + 2]
        pol = tm.main(av + ["--dir", str(tmp_path / key), "--params", json.dumps(params)])
        torch.cuda.synchronize()
        csv = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path / key) for f in fs if f == "scalars.csv"]
        runs[key] = (snapshot(pol), open(csv[0], "rb").read())
    assert differing(runs["given"][0], runs["omitted"][0]) == [] and runs["given"][1] == runs["omitted"][1]
    assert runs["given"][1].startswith(b"tag,step,value\n")
