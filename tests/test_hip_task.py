"""The analytic control task on the device (csrc/task.hip; mobody_amd/task.py): `mobody_task_step` per element against the
fp64 restatement (tests/task_ref.py) within the derived bound, `mobody_task_evaluate` bit for bit against the composition of
`mobody_mlp3_forward`, `mobody_task_step` under the carried mask and tests/model_eval_ref.py's accounting, `mobody_task_collect`
against `mobody_task_step` driven by the restatement's controller, the refusals, and `--synthetic 2` end to end."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import model_eval_ref as ref
import task_ref as R
from test_hip_fqe import differing, packed_policy, snapshot
from test_hip_model_eval import assert_state_bits, lengths_from_flags

pytestmark = pytest.mark.gpu

SEED, CALL0 = 20261, 7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_tables = []            # the device tables a MobodyTaskParams points to stay alive for the module


def device_params(p, dev, sigma=None):
    """MobodyTaskParams of a restatement parameter dict."""
    from mobody_amd import _lib, ops
    mu = torch.from_numpy(np.asarray(p["mu"], np.float32)).to(dev)
    gain = torch.from_numpy(np.asarray(p["gain"], np.float32)).to(dev)
    bm = torch.from_numpy(p["bmat"]).to(dev).contiguous()
    _tables.append((mu, gain, bm))
    kind = next(k for k in _lib.TERM_IDS if k in p["task"])
    return ops.task_params(p["S"], p["A"], _lib.TERM_IDS[kind], mu, gain, bm, f=p["f"], grav=p["grav"], dt=R.DT, g=R.G, c=R.C,
                           lam=R.LAM, k=R.K, h=R.H, sigma=p["sigma"] if sigma is None else sigma, alive_bonus=R.ALIVE_BONUS,
                           ctrl_cost=R.CTRL_COST, max_action=p["max_action"])


def T(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def bits(t):
    return t.contiguous().view(torch.uint8)


# ---- 1. mobody_task_step against fp64 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,A,task,why", R.STEP_SHAPES, ids=[f"S{s[0]}A{s[1]}" for s in R.STEP_SHAPES])
def test_step_against_fp64_per_element(S, A, task, why, dev):
    from mobody_amd import ops
    flags = []
    for B in R.step_rows(S):
        p, s, a, n = R.step_case(S, A, task, B)
        want = R.step(p, s, a, n)
        got = ops.task_step(device_params(p, dev), T(s, dev), T(a, dev), noise=T(n, dev))
        nxt, rew = got["next_obs"].cpu().numpy().astype(np.float64), got["reward"].cpu().numpy().astype(np.float64)
        term = got["terminal"].cpu().numpy() != 0
        e_n, b_n = np.abs(nxt - want["next"]), R.bound(p, want["mag_next"])
        e_r, b_r = np.abs(rew - want["reward"]), R.bound(p, want["mag_reward"])
        print(f"task_step S={S} A={A} B={B} ({why}): next err/bound {float((e_n / b_n).max()):.4f}, reward {float((e_r / b_r).max()):.4f}")
        assert (e_n <= b_n).all() and (e_r <= b_r).all()
        near = R.near_threshold(p, want)
        assert near.sum() <= 0.01 * B
        assert np.array_equal(term[~near], want["terminal"][~near])
        flags.append(term)
    flags = np.concatenate(flags)
    assert flags.any() and not flags.all()


def test_step_device_noise_alive_mask_and_in_place(dev):
    """noise = NULL has the bits of the same call fed mobody_rng_normal(seed, 4, call) (the call id through call_dev as well); a dead
    row is computed and its flag is 0; next_obs may be obs."""
    from mobody_amd import ops
    S, A, task, _ = R.STEP_SHAPES[2]
    B = 257
    p, s, a, _ = R.step_case(S, A, task, B)
    dp = device_params(p, dev)
    s_d, a_d = T(s, dev), T(a, dev)
    noise = ops.rng_normal(SEED, 4, CALL0 + 3, B * S, dev).reshape(B, S)
    fed = ops.task_step(dp, s_d, a_d, noise=noise)
    own = ops.task_step(dp, s_d, a_d, seed=SEED, call=CALL0 + 3)
    word = ops.task_step(dp, s_d, a_d, seed=SEED, call=CALL0, call_dev=torch.tensor([3], dtype=torch.int64, device=dev))
    other = ops.task_step(dp, s_d, a_d, seed=SEED, call=CALL0 + 4)
    for k in fed:
        assert torch.equal(bits(fed[k]), bits(own[k])) and torch.equal(bits(fed[k]), bits(word[k])), k
    assert not torch.equal(bits(fed["next_obs"]), bits(other["next_obs"]))
    quiet = ops.task_step(device_params(p, dev, sigma=0.0), s_d, a_d, seed=SEED, call=CALL0)          # sigma == 0 draws nothing
    want = R.step(dict(p, sigma=0.0), s, a)
    assert np.abs(quiet["next_obs"].cpu().numpy() - want["next"]).max() < 1e-5
    alive = torch.ones(B, dtype=torch.uint8, device=dev)
    alive[::3] = 0
    masked = ops.task_step(dp, s_d, a_d, noise=noise, alive=alive)
    assert torch.equal(bits(masked["next_obs"]), bits(fed["next_obs"])) and torch.equal(bits(masked["reward"]), bits(fed["reward"]))
    assert torch.equal(masked["terminal"], fed["terminal"] * alive) and int(fed["terminal"][::3].sum()) > 0
    inplace = s_d.clone()
    ops.task_step(dp, inplace, a_d, noise=noise, out=dict(next_obs=inplace))
    assert torch.equal(bits(inplace), bits(fed["next_obs"]))


# ---- 2. mobody_task_evaluate against the composition ---------------------------------------------------------------------------
ES, EA, ETASK = 17, 6, "walker2d-medium-v2"


def eval_params():
    return R.params(ES, EA, ETASK, f=2.0, gain=[0.5] + [1.0] * (EA - 1))


def eval_init(B, dev):
    """Start states around mu; every third row leans at or past the walker's |angle| < 1 edge (the predicate reads the NEXT state):
    under a policy net such a row falls within a few steps, under the built-in controller only the rows past about 1.03 do."""
    rng = np.random.default_rng(11)
    p = eval_params()
    s = p["mu"] + 0.05 * rng.standard_normal((B, ES)).astype(np.float32)
    lean = np.arange(B) % 3 == 0
    s[lean, 1] = rng.uniform(0.93, 1.08, int(lean.sum())) * rng.choice([-1.0, 1.0], int(lean.sum()))
    return T(s.astype(np.float32), dev)


def compose(dp, net, head, init, H, discount=1.0):
    """mlp3_forward (out_mode 1; [:, :A] at head 1) + mobody_task_step under the carried mask + the accounting of model_eval_ref."""
    from mobody_amd import ops
    B, dev = init.shape[0], init.device
    st, obs, terms = ref.new_state(B), init, []
    for t in range(H):
        out = ops.mlp3_forward(net.blob, ES, net.out_dim, 1, obs, out_mode=1, max_action=1.0, blob_T=net.blob_T, precision=net.precision)[0]
        act = out[:, :EA].contiguous()
        alive = T(st["alive"].astype(np.uint8), dev)
        r = ops.task_step(dp, obs, act, alive=alive, seed=SEED, call=CALL0 + t)
        term = r["terminal"].cpu().numpy() != 0
        terms.append(term)
        ref.account(st, r["reward"].cpu().numpy(), np.zeros(B, np.float32), term, discount)
        obs = r["next_obs"]
    return st, obs, np.array(terms)


def workspace_floats(A, B, head):
    r4 = lambda n: (n + 3) // 4 * 4
    return r4(B * A) + (r4(2 * B * A) if head == 1 else 0)


GUARD = 64


def fused(dp, net, head, init, H, discount=1.0, state=None, resume=False, call0=CALL0, call_dev=None, **ctrl):
    """mobody_task_evaluate on a row state and a workspace pre-filled with a byte pattern, NaN sentinels behind the workspace."""
    from mobody_amd import _lib, ops
    B, dev = init.shape[0], init.device
    if state is None:
        state = ops.eval_state(B, ES, dev)
        for v in state.values():
            v.view(torch.uint8).fill_(0xA5)
    need = workspace_floats(EA, B, head)
    blk = _lib.block(_lib.MobodyTaskEval, p=dp, B=B, head=head)
    assert ops.load().mobody_task_evaluate_workspace(C.byref(blk)) == need
    ws = torch.empty(need + GUARD, dtype=torch.float32, device=dev)
    ws.view(torch.uint8).fill_(0xA5)
    ws[need:] = float("nan")
    guard = ws[need:].clone()
    got = ops.task_evaluate(dp, None if net is None else net.blob, head, None if resume else init, H, SEED, call0, state, discount=discount,
                            resume=resume, ws=ws, policy_blob_T=None if net is None else net.blob_T,
                            precision=0 if net is None else net.precision, call_dev=call_dev, **ctrl)
    assert got is ws and torch.equal(ws[need:].view(torch.int32), guard.view(torch.int32)), "a launch wrote behind the workspace"
    return state


def same_bytes(a, b):
    return [k for k in a if not torch.equal(bits(a[k]), bits(b[k]))]


@pytest.mark.parametrize("discount", [1.0, 0.99])
@pytest.mark.parametrize("head", [0, 1])
def test_evaluate_equals_the_composition_bit_for_bit(head, discount, mfma, dev):
    dp = device_params(eval_params(), dev)
    net, _ = packed_policy(ES, EA, head, dev, mfma)
    init = eval_init(65, dev)
    disc = float(np.float32(discount))
    st, obs, terms = compose(dp, net, head, init, 7, disc)
    length = lengths_from_flags(terms)
    assert st["alive"].any() and not st["alive"].all() and len(set(length.tolist())) >= 3      # fallen and surviving rows, by the composition
    got = fused(dp, net, head, init, 7, disc)
    assert_state_bits(got, st, obs)
    assert np.array_equal(st["length"], length) and np.isfinite(st["ret"]).all() and float(got["pen_sum"].abs().max()) == 0.0
    if discount == 1.0:                                      # the summary serves the row state unchanged
        from mobody_amd import ops
        w = ops.eval_summary(got, 1).cpu()[:8].tolist()
        assert w[4] == pytest.approx(float(st["ret"].astype(np.float64).mean()), rel=1e-5) and w[5] == pytest.approx(length.mean(), rel=1e-6)
        assert w[6] == 0.0 and w[7] == pytest.approx(st["alive"].mean(), rel=1e-6)


def test_evaluate_row_counts_resume_and_call_word(dev):
    dp = device_params(eval_params(), dev)
    net, _ = packed_policy(ES, EA, 1, dev)
    for B in (1, 257):
        init = eval_init(B, dev)
        st, obs, _ = compose(dp, net, 1, init, 7)
        assert_state_bits(fused(dp, net, 1, init, 7), st, obs)
    init = eval_init(65, dev)
    one = fused(dp, net, 1, init, 7)
    two = fused(dp, net, 1, init, 3)
    fused(dp, net, 1, init, 4, state=two, resume=True, call0=CALL0 + 3)
    three = fused(dp, net, 1, init, 3, call_dev=torch.zeros(1, dtype=torch.int64, device=dev))
    fused(dp, net, 1, init, 4, state=three, resume=True, call_dev=torch.tensor([3], dtype=torch.int64, device=dev))
    assert same_bytes(one, two) == [] and same_bytes(one, three) == []
    zero = fused(dp, net, 1, init, 0)                       # H == 0 only initialises the row state
    assert_state_bits(zero, ref.new_state(65), init)


@pytest.mark.parametrize("head", [0, 1, 2])
def test_captured_chunk_replayed_three_times_equals_one_eager_call(head, dev):
    from mobody_amd import ops
    dp = device_params(eval_params(), dev)
    net = None if head == 2 else packed_policy(ES, EA, head, dev)[0]
    ctrl = dict(ctrl=1, ctrl_push=1.0, ctrl_eps=0.1) if head == 2 else {}
    init = eval_init(65, dev)
    eager = fused(dp, net, head, init, 9, 0.99, **ctrl)
    st = fused(dp, net, head, init, 0, 0.99, **ctrl)
    ws = torch.empty(workspace_floats(EA, 65, head) + GUARD, dtype=torch.float32, device=dev)
    ctr = torch.full((1,), CALL0, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                # (ops directly: the guard checks of fused() synchronise)
        ops.task_evaluate(dp, None if net is None else net.blob, head, None, 3, SEED, 0, st, discount=0.99, resume=True, ws=ws,
                          policy_blob_T=None if net is None else net.blob_T, call_dev=ctr, **ctrl)
        ops.counter_add(ctr, 3)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert same_bytes(eager, st) == [] and int(ctr[0]) == CALL0 + 9
    assert len(set(eager["length"].tolist())) >= 2


def test_head2_equals_the_restated_controller_through_task_step(dev):
    from mobody_amd import ops
    p = eval_params()
    dp = device_params(p, dev)
    init = eval_init(65, dev)
    push, eps_a = R.CONTROLLERS["medium"]
    st, obs, terms = ref.new_state(65), init, []
    for t in range(7):
        na = ops.rng_normal(SEED, 5, CALL0 + t, 65 * EA, dev).reshape(65, EA).cpu().numpy()
        act = T(R.controller32(p, obs.cpu().numpy(), push, eps_a, na), dev)
        r = ops.task_step(dp, obs, act, alive=T(st["alive"].astype(np.uint8), dev), seed=SEED, call=CALL0 + t)
        term = r["terminal"].cpu().numpy() != 0
        terms.append(term)
        ref.account(st, r["reward"].cpu().numpy(), np.zeros(65, np.float32), term, 1.0)
        obs = r["next_obs"]
    assert st["alive"].any() and not st["alive"].all()
    assert_state_bits(fused(dp, None, 2, init, 7, ctrl=1, ctrl_push=push, ctrl_eps=eps_a), st, obs)
    # the random controller: uniform actions, another run
    rand = fused(dp, None, 2, init, 7, ctrl=0)
    assert same_bytes(rand, fused(dp, None, 2, init, 7, ctrl=0)) == [] and "ret" in same_bytes(rand, fused(dp, None, 2, init, 7, ctrl=1))


# ---- 3. mobody_task_collect ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["medium-expert", "random"])
def test_collect_equals_task_step_driven_by_the_restated_controller(kind, dev):
    from mobody_amd import ops
    from mobody_amd.task import controller_of
    p = R.from_env("hopper-kinematic", "hard", "target")
    dp = device_params(p, dev)
    S, A, lanes, L, limit, init_std = p["S"], p["A"], 9, 12, 5, 0.12
    ctrl, push, eps, split = controller_of(kind, lanes)
    got = ops.task_collect(dp, lanes, L, limit, ctrl, push, eps, split, init_std, SEED, call0=CALL0)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    mu = T(p["mu"], dev)
    start = lambda e: (mu + np.float32(init_std) * ops.rng_normal(SEED, 6, e, lanes * S, dev).reshape(lanes, S))
    obs, age, ep = start(0), np.zeros(lanes, int), np.zeros(lanes, int)
    n_term = n_cut = 0
    for t in range(L):
        rows = np.arange(lanes) * L + t
        if kind == "random":
            # 2 u - 1 with u = (x >> 8) 2^-24 + 2^-25 of word i & 3 of counter i >> 2, i = b A + j: mobody_rng_index with bound 2^24
            # returns exactly x >> 8 of that word (the project's other reader of the Philox stream, a kernel of its own)
            x = ops.rng_index(SEED, 5, CALL0 + t, lanes * A, 1 << 24, dev).reshape(lanes, A).cpu().numpy().astype(np.float32)
            u01 = (x * np.float32(2.0 ** -24)).astype(np.float32) + np.float32(2.0 ** -25)
            act = T((np.float32(2.0) * u01 - np.float32(1.0)).astype(np.float32), dev)
        else:
            na = ops.rng_normal(SEED, 5, CALL0 + t, lanes * A, dev).reshape(lanes, A).cpu().numpy()
            o = obs.cpu().numpy()
            act = T(np.concatenate([R.controller32(p, o[:split], push[0], eps[0], na[:split]),
                                    R.controller32(p, o[split:], push[1], eps[1], na[split:])]), dev)
        r = ops.task_step(dp, obs, act, seed=SEED, call=CALL0 + t)
        for k, v in (("observations", obs), ("actions", act), ("next_observations", r["next_obs"]), ("rewards", r["reward"])):
            assert np.array_equal(got[k][rows].view(np.int32), v.cpu().numpy().view(np.int32)), (k, t)
        term = r["terminal"].cpu().numpy() != 0
        assert np.array_equal(got["terminals"][rows] != 0, term), t
        age += 1
        reset = term | (age >= limit)
        n_term, n_cut = n_term + int(term.sum()), n_cut + int((reset & ~term).sum())
        ep += reset
        nxt = r["next_obs"].clone()
        for b in np.flatnonzero(reset):
            nxt[b] = start(int(ep[b]))[b]
        age[reset] = 0
        obs = nxt
    # from the reference side: terminations, time-limit restarts, and lanes whose last episode is cut by the lane's end alone
    assert n_term > 0 and n_cut > 0 and (age > 0).any()
    assert np.abs(got["actions"]).max() <= 1.0
    if kind == "random":
        a = got["actions"]
        assert abs(float(a.mean())) < 0.2 and 0.2 < float(a.std()) < 0.8 and len(np.unique(a)) == a.size


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field_and_touch_nothing(dev):
    from mobody_amd import _lib, ops
    lib = ops.load()
    p = eval_params()
    B = 8
    buf = {k: torch.empty(n, dtype=torch.float32, device=dev) for k, n in
           (("obs", B * ES), ("act", B * EA), ("next_obs", B * ES), ("reward", B), ("terminal", B), ("ws", 256), ("ret", B))}
    for v in buf.values():
        v.view(torch.uint8).fill_(0xA5)
    before = {k: v.clone() for k, v in buf.items()}
    ptr = lambda k: buf[k].data_ptr()

    def params(**over):
        dp = device_params(p, dev)
        for k, v in over.items():
            setattr(dp, k, v)
        return dp

    def refused(entry, blk, *words):
        assert getattr(lib, entry)(C.byref(blk), None) == -1, entry
        msg = lib.mobody_last_error().decode()
        assert msg.startswith(entry + ":") or msg.startswith("mobody_mlp_layout:"), msg
        for w in words:
            assert w in msg, (w, msg)

    step = lambda dp=None, **f: _lib.block(_lib.MobodyTaskStep, p=dp or params(), **dict(
        dict(obs=ptr("obs"), act=ptr("act"), B=B, next_obs=ptr("next_obs"), reward=ptr("reward"), terminal=ptr("terminal")), **f))
    refused("mobody_task_step", _lib.MobodyTaskStep(struct_bytes=C.sizeof(_lib.MobodyTaskStep) - 1), "struct_bytes")
    refused("mobody_task_step", step(params(S=2)), "S 2")
    refused("mobody_task_step", step(params(S=257)), "S 257")
    refused("mobody_task_step", step(params(A=0)), "A 0")
    refused("mobody_task_step", step(params(A=65)), "A 65")
    refused("mobody_task_step", step(params(task=9)), "task")
    refused("mobody_task_step", step(params(task=6)), "pen")
    refused("mobody_task_step", step(params(max_action=0.0)), "max_action")
    refused("mobody_task_step", step(B=-1), "B < 0")
    for f in ("mu", "gain", "bmat"):
        refused("mobody_task_step", step(params(**{f: None})), "null pointer " + f)
    for f in ("obs", "act", "next_obs", "reward", "terminal"):
        refused("mobody_task_step", step(**{f: None}), "null pointer " + f)
    assert lib.mobody_task_step(C.byref(step(B=0, obs=None)), None) == 0

    ev = lambda dp=None, **f: _lib.block(_lib.MobodyTaskEval, p=dp or params(), **dict(
        dict(policy_blob=ptr("ws"), init_obs=ptr("obs"), B=B, H=2, head=0, discount=1.0, obs_state=ptr("next_obs"), alive=ptr("terminal"),
             ret=ptr("ret"), pen_sum=ptr("ret"), disc=ptr("ret"), length=ptr("ret"), workspace=ptr("ws")), **f))
    refused("mobody_task_evaluate", _lib.MobodyTaskEval(struct_bytes=8), "struct_bytes")
    refused("mobody_task_evaluate", ev(params(S=2)), "S 2")
    refused("mobody_task_evaluate", ev(head=3), "head 3")
    refused("mobody_task_evaluate", ev(head=-1), "head -1")
    refused("mobody_task_evaluate", ev(head=2, ctrl=2), "ctrl 2")
    refused("mobody_task_evaluate", ev(resume=2), "resume")
    refused("mobody_task_evaluate", ev(discount=0.0), "discount")
    refused("mobody_task_evaluate", ev(H=-1), "H < 0")
    refused("mobody_task_evaluate", ev(precision=7), "precision")
    refused("mobody_task_evaluate", ev(precision=4), "T blob")
    for f in ("policy_blob", "init_obs", "obs_state", "alive", "ret", "pen_sum", "disc", "length", "workspace"):
        refused("mobody_task_evaluate", ev(**{f: None}), "null pointer " + f)
    assert lib.mobody_task_evaluate_workspace(C.byref(_lib.MobodyTaskEval(struct_bytes=8))) == -1

    co = lambda dp=None, **f: _lib.block(_lib.MobodyTaskCollect, p=dp or params(), **dict(
        dict(lanes=2, split=1, L=2, time_limit=5, ctrl=(C.c_int32 * 2)(1, 1), observations=ptr("obs"), actions=ptr("act"),
             next_observations=ptr("next_obs"), rewards=ptr("reward"), terminals=ptr("terminal"), workspace=ptr("ws")), **f))
    refused("mobody_task_collect", _lib.MobodyTaskCollect(struct_bytes=8), "struct_bytes")
    refused("mobody_task_collect", co(params(S=1)), "S 1")
    refused("mobody_task_collect", co(lanes=-1), "lanes")
    refused("mobody_task_collect", co(L=-1), "L < 0")
    refused("mobody_task_collect", co(time_limit=0), "time_limit")
    refused("mobody_task_collect", co(split=3), "split")
    refused("mobody_task_collect", co(ctrl=(C.c_int32 * 2)(1, 5)), "ctrl 5")
    for f in ("observations", "actions", "next_observations", "rewards", "terminals", "workspace"):
        refused("mobody_task_collect", co(**{f: None}), "null pointer " + f)
    torch.cuda.synchronize()
    for k, v in buf.items():
        assert torch.equal(bits(v), bits(before[k])), k


# ---- 5. Task.evaluate and the CLI ------------------------------------------------------------------------------------------------------
def test_task_class_chunked_evaluation_and_reference_points(dev):
    """Task.evaluate: the chunk graph equals the eager call, two calls agree bit for bit, and the built-in controllers order as the
    task is built for: random falls, expert survives the source, and falls under `kinematic hard`."""
    from mobody_amd.task import Task, TaskSpec
    src = Task(TaskSpec.from_env("hopper-kinematic", "hard", "source"), dev, seed=3)
    tar = Task(TaskSpec.from_env("hopper-kinematic", "hard", "target"), dev, seed=3)
    net, _ = packed_policy(11, 3, 0, dev)
    eager = src.evaluate(net, 0, 33, horizon=9, chunk=0)
    graph = src.evaluate(net, 0, 33, horizon=9, chunk=3)
    again = src.evaluate(net, 0, 33, horizon=9, chunk=3)
    assert src.eval_captures == 1
    for k in ("returns", "lengths", "alive"):
        assert torch.equal(bits(eager[k]), bits(graph[k])) and torch.equal(bits(eager[k]), bits(again[k])), k
    assert eager["return_mean"] == graph["return_mean"] == pytest.approx(float(eager["returns"].double().mean()), rel=1e-5)
    rand = src.evaluate(None, 2, 64, horizon=300, controller="random")
    exp_src = src.evaluate(None, 2, 64, horizon=300, controller="expert")
    exp_tar = tar.evaluate(None, 2, 64, horizon=300, controller="expert")
    med_tar = tar.evaluate(None, 2, 64, horizon=300, controller="medium")
    print("hopper kinematic hard, 64 episodes of 300 steps:", {k: (v["return_mean"], v["length_mean"], v["alive_frac"]) for k, v in
                                                               dict(random=rand, expert_src=exp_src, expert_tar=exp_tar, medium_tar=med_tar).items()})
    assert rand["length_mean"] < 200 and rand["alive_frac"] == 0.0
    assert exp_src["alive_frac"] == 1.0 and exp_src["length_mean"] == 300.0
    assert exp_tar["length_mean"] < 200 and med_tar["alive_frac"] > 0.5


TAGS = ("test/source return", "test/target return", "test/target episode length", "test/target normalized score")
LEARN_STEPS = 5000


def scalars(out_dir):
    csv = [f for d, _, fs in os.walk(out_dir) for f in (os.path.join(d, x) for x in fs) if f.endswith("scalars.csv")]
    return [(r[0], int(r[1]), float(r[2])) for r in (ln.strip().split(",") for ln in open(csv[0]).readlines()[1:])]


def cli(tmp_path, synthetic, steps, eval_freq, rows=20000):
    return ["--policy", "TD3_BC", "--env", "hopper-friction", "--shift_level", "2.0", "--mode", "3", "--seed", "1", "--synthetic", str(synthetic),
            "--tartype", "expert", "--srctype", "expert", "--rng", "device", "--src_rows", str(rows), "--tar_rows", str(rows),
            "--max_step", str(steps), "--eval_freq", str(eval_freq), "--log_every", str(steps), "--dir", str(tmp_path),
            "--params", json.dumps(dict(batch_size=256, graph=1))]


def test_cli_synthetic2_logs_true_returns_and_learns(tmp_path, monkeypatch, dev):
    """--synthetic 2 end to end.  The learning condition of the issue: with R0 the untrained policy's true target return and R_data
    the data's mean episode return, the trained policy reaches R > R0 + 0.5 (R_data - R0) (figures in DESIGN 5zf)."""
    from mobody_amd import train_mobody as tm
    from mobody_amd.algo import utils
    from mobody_amd.task import Task, TaskSpec
    made = []
    init = utils.ReplayBuffer.__init__
    monkeypatch.setattr(utils.ReplayBuffer, "__init__", lambda self, *a, **k: (init(self, *a, **k), made.append(self))[0])
    tar = Task(TaskSpec.from_env("hopper-friction", "2.0", "target"), dev, seed=1)
    pol0 = tm.main(cli(tmp_path / "zero", 2, 0, 1, rows=4000))
    r0 = pol0.evaluate_in_task(tar, 32, 1000)["return_mean"]
    del made[:]
    pol = tm.main(cli(tmp_path / "run", 2, LEARN_STEPS, LEARN_STEPS // 2))
    torch.cuda.synchronize()
    rows = scalars(tmp_path / "run")
    tags = {t for t, _, _ in rows}
    assert set(TAGS) | {"data/source return", "data/target return"} <= tags
    last = {t: v for t, s, v in rows if s == LEARN_STEPS}
    r_data = [v for t, _, v in rows if t == "data/target return"][0]

    def state():
        s = snapshot(pol)
        for i, rb in enumerate(made):
            s.update({"buffer%d.%s" % (i, k): v for k, v in snapshot(rb).items()})
        s["torch.cpu_rng"], s["torch.cuda_rng"] = torch.get_rng_state(), torch.cuda.get_rng_state()
        return s

    before = state()
    ev = pol.evaluate_in_task(tar, 32, 1000)
    torch.cuda.synchronize()
    bad = differing(before, state())
    assert any(k.endswith("._draws") for k in before) and bad == [], " ".join(bad)      # Task.evaluate moves no training state
    assert ev["return_mean"] == last["test/target return"] and ev["length_mean"] == last["test/target episode length"]
    r = ev["return_mean"]
    print(f"--synthetic 2 TD3_BC hopper-friction 2.0 expert/expert: R0 {r0:.1f}, R_data {r_data:.1f}, R {r:.1f} after {LEARN_STEPS} steps; "
          f"normalized score {last['test/target normalized score']:.1f}, source return {last['test/source return']:.1f}")
    assert all(np.isfinite(v) for _, _, v in rows)
    assert r > r0 + 0.5 * (r_data - r0)


def test_cli_synthetic1_writes_none_of_the_new_tags(tmp_path):
    from mobody_amd import train_mobody as tm
    tm.main(cli(tmp_path, 1, 8, 4, rows=600))
    tags = {t for t, _, _ in scalars(tmp_path)}
    assert not tags & (set(TAGS) | {"data/source return", "data/target return"})
