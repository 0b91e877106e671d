"""config['f16_guard'] = 'fallback' in every algorithm class: TD3_BC, IQL, DARA, IGDF and BOSA's critic / actor stage.

tests/test_hip_health_mirror.py covers MOBODY.  The subclasses carry fallback code of their own -- _extra_named() (the nets a class
runs at the configured MFMA mode besides the twin-Q, its target and the policy), IGDF dropping its info graph, BOSA's
_health_check_stage2 and the precision entry of its graph key -- and this file runs it.

The planted critic: W2[n][k] of critic member 0 at 255.875 - 2.5 lr, every reward 1e4.  The TD target then exceeds Q on every row
(IQL's r + gamma V(s'), DARA's relabeled r +- 0.2 and IGDF's positive row weights change nothing of that), so dL/dz2[.][n] has the
sign of -W3[n]; n is a hidden unit with W3[n] > 0, k the layer-1 unit of largest bias: Adam moves the weight up by ~lr per step
(exactly lr in the first) and it crosses 255.875 in the third -- after a graph of the f16x2 step exists.  The step the message
names is asserted (a precondition of the case).  Where no sign can be argued (BOSA's masked conservative critic, V's expectile
loss, a classifier head, a contrastive encoder) four PAIRS are planted: in hidden unit n, +(255.875 - lr / 2) on the layer-1 unit
of largest bias and -(255.875 - lr / 2) on the one of second largest.  Both inputs are >= 0, so both gradients have the sign of
dL/dz2[.][n]: the two weights move the same way by lr in the first step, and one of them moves outwards whatever that sign is
(the unit is live wherever the first input exceeds the second).  That at least one crossed is asserted first.

Comparisons are bit for bit.  The eager fallback run against a fresh bf16x3 object that loaded the state a 'raise' twin froze.
The run with graph = 1 against the same run whose steps are enqueued eagerly: the step's own closures outside a capture, which is
what tests/test_hip_{td3bc,iql,dara,igdf}.py call the eager steps of a replayed run (train()'s eager path itself forms Adam's bias
corrections on the host and is not bit-comparable with any replay, fallback or not: tests/test_hip_iql.py).  A stale f16x2 graph
replayed against bf16x3 planes cannot pass that."""
import contextlib
import gc
import re
import warnings

import numpy as np
import pytest
import torch

import dara_ref as DR
import golden_util as gu
import igdf_ref as GR
import iql_ref as IR
from test_hip_health_mirror import _clean_words, rows            # noqa: F401  (_clean_words: autouse here too)

pytestmark = pytest.mark.gpu

S, A, BS = 17, 6, 64
LR = 3e-4
LIMIT = 255.875
EVERY = 8                       # health cadence of these tests: check points at total_it = 1, 9, 17, ...
ALGOS = ("td3_bc", "iql", "dara", "igdf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def cadence(monkeypatch):
    import mobody_amd.algo.offline_offline.bosa as bosa
    import mobody_amd.algo.offline_offline.iql as iql
    import mobody_amd.algo.offline_offline.mobody as mob
    import mobody_amd.algo.offline_offline.td3_bc as td3
    for m in (mob, td3, iql, bosa):
        monkeypatch.setattr(m, "REFRESH_EVERY", EVERY)


BUILT = []                      # every object a test made


@pytest.fixture(autouse=True)
def _no_graph_is_left_to_the_collector():
    """The tests hang closures on their objects (watch, enqueue_instead_of_replaying): reference cycles, so the objects -- and the
    HIP graphs they hold -- would be freed by the cyclic collector, whenever it runs.  If it runs while a later test captures a
    graph, destroying a graph there is an error the runtime answers by aborting the process.  So each test takes its closures
    off again and drops its graphs here, outside any capture (and collects what earlier tests left before it captures one)."""
    gc.collect()
    yield
    torch.cuda.synchronize()
    for pol in BUILT:
        for name in ("_health_check", "_graph_segments"):
            pol.__dict__.pop(name, None)
        pol._graph = None
        if hasattr(pol, "_info_graph"):
            pol._info_graph = None
        if hasattr(pol, "_s2_graphs"):
            pol._s2_graphs, pol._s2_graph_key = {}, None
    del BUILT[:]
    gc.collect()


def build(algo, dev, guard, mfma, **over):
    from mobody_amd.algo.offline_offline.dara import DARA
    from mobody_amd.algo.offline_offline.igdf import IGDF
    from mobody_amd.algo.offline_offline.iql import IQL
    from mobody_amd.algo.offline_offline.td3_bc import TD3BC
    kw = dict(mfma=mfma, f16_guard=guard, **over)
    torch.manual_seed(3)
    cls, cfg = {"td3_bc": (TD3BC, gu.policy_cfg), "iql": (IQL, IR.iql_cfg), "dara": (DARA, DR.dara_cfg),
                "igdf": (IGDF, lambda *a, **k: GR.igdf_cfg(*a, info_update_step=3, **k))}[algo]
    BUILT.append(cls(cfg(S, A, **kw), dev))
    return BUILT[-1]


def assert_lr(pol):
    assert pol.q_optimizer.lr == LR and pol.v_optimizer.lr == LR


def copy_into_clone(target, net):
    """The target stays what the constructor made it, a clone() that never loaded a state dict (as in a run without a checkpoint):
    the fallback has to cope with that."""
    target.blob.copy_(net.blob)
    target.blob_T.copy_(net.blob_T)


def plant_critic(pol):
    sd = {k: v.clone() for k, v in pol.q_funcs.state_dict().items()}
    n = int(torch.argmax(sd["network1.network.4.weight"][0]))
    k = int(torch.argmax(sd["network1.network.0.bias"]))
    assert float(sd["network1.network.4.weight"][0, n]) > 0
    sd["network1.network.2.weight"][n, k] = LIMIT - 2.5 * LR          # nn.Linear layout [out][in]
    pol.q_funcs.load_state_dict(sd)
    copy_into_clone(pol.target_q_funcs, pol.q_funcs)


def plant_pairs(net, lr, pre=None):
    """Four pairs +-(255.875 - lr / 2) in W2 of member 0 of `net` (see the module docstring)."""
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    pre = net.prefixes[0] if pre is None else pre
    k1, k2 = (int(x) for x in torch.argsort(sd[pre + "network.0.bias"], descending=True)[:2])
    for n in (3, 77, 150, 222):
        sd[pre + "network.2.weight"][n, k1] = LIMIT - lr / 2
        sd[pre + "network.2.weight"][n, k2] = -(LIMIT - lr / 2)
    net.load_state_dict(sd)


def all_nets(pol):
    return (pol.q_funcs, pol.target_q_funcs, pol.policy) + tuple(pol._extra_nets())


def all_opts(pol):
    o = [pol.q_optimizer, pol.policy_optimizer, pol.v_optimizer, pol.classifier.opt_sa, pol.classifier.opt_sas]
    if hasattr(pol, "info_optimizer"):
        o += [pol.info_optimizer.sa, pol.info_optimizer.ss]
    return o


def bits(t):
    return t.contiguous().view(torch.int32)


def after_the_fallback(pol, nets, opts, hyp=None):
    """What holds the moment _health_check has fallen back (before the next step touches anything)."""
    from mobody_amd import ops
    torch.cuda.synchronize()
    assert pol.precision == 3 and (hyp is None or hyp.precision == 3)
    for n in nets:
        assert n.precision == 3
        fresh = ops.mlp_transpose(n.blob, n.in_dim, n.out_dim, n.members, precision="bf16x3")
        assert fresh.shape == n.blob_T.shape and torch.equal(bits(fresh), bits(n.blob_T)), n.prefixes
        assert bool(torch.isfinite(n.blob).all())
    mask, _ = ops.health_read(ops.health_bound(pol.device))
    assert mask == 0
    for o in opts:
        assert bool(torch.isfinite(o.m).all()) and bool(torch.isfinite(o.v).all())


def watch(pol, fell, nets=all_nets, opts=all_opts, hyp=lambda p: None):
    """Run after_the_fallback inside the train() call whose health check fell back; fell collects that call's total_it."""
    real = pol._health_check

    def check():
        before = pol.precision
        real()
        if pol.precision != before:
            after_the_fallback(pol, nets(pol), opts(pol), hyp(pol))
            fell.append(pol.total_it)
    pol._health_check = check


def fault_step(rec):
    msgs = [str(w.message) for w in rec if "bf16x3" in str(w.message)]
    assert len(msgs) == 1, msgs
    assert "F16_RANGE" in msgs[0]
    m = re.search(r"at Adam step (\d+)", msgs[0])
    return msgs[0], int(m.group(1)) if m else None


def same_state(x, y):
    torch.cuda.synchronize()
    for i, (n, m) in enumerate(zip(all_nets(x), all_nets(y))):
        assert torch.equal(n.blob, m.blob), ("blob", i, n.prefixes)
        assert torch.equal(bits(n.blob_T), bits(m.blob_T)), ("T blob", i, n.prefixes)
        assert n.precision == m.precision == 3
    for i, (o, p) in enumerate(zip(all_opts(x), all_opts(y))):
        assert torch.equal(o.m, p.m) and torch.equal(o.v, p.v) and o.t == p.t, ("optimizer", i)


# ---- the planted critic, eager ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ALGOS)
def test_fallback_continues_in_bf16x3_from_the_frozen_state(algo, cadence, dev, tmp_path):
    from mobody_amd import ops
    src, tar = rows(501, dev), rows(502, dev)
    # the frozen state, from a 'raise' twin: calls 1 .. 8, the check of call 9 raises
    a = build(algo, dev, "raise", "f16x2")
    assert_lr(a)
    plant_critic(a)
    with pytest.raises(FloatingPointError, match="q_funcs") as ei:
        for _ in range(EVERY + 1):
            a.train(src, tar, BS, None, None)
    assert a.total_it == EVERY + 1 and "F16_RANGE" in str(ei.value)
    prefix = str(tmp_path / "frozen")
    a.save(prefix)
    target = a.target_q_funcs.state_dict()
    ops.health_clear()
    # the run under test
    f = build(algo, dev, "fallback", "f16x2")
    plant_critic(f)
    fell = []
    watch(f, fell)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        for _ in range(EVERY + 1 + 20):
            f.train(src, tar, BS, None, None)
            assert f.total_it > EVERY or f.precision == 4
    msg, step = fault_step(rec)
    print(algo, "|", msg[:160])
    assert fell == [EVERY + 1] and "q_funcs" in msg and step == 3, "precondition: the planted weight crosses in the third step"
    assert f.mfma == "bf16x3" and f.config["mfma"] == "bf16x3" and f.q_optimizer.t == 3 + 21
    assert all(np.isfinite(x) for x in f.losses())
    # a fresh bf16x3 object with the frozen state, the same targets, counts and rows
    b = build(algo, dev, "raise", "bf16x3")
    b.load(prefix)
    b.target_q_funcs.load_state_dict(target)
    b.total_it = EVERY
    if algo == "dara":
        b.classifier._calls = a.classifier._calls               # the noise stream's call id
    assert b.q_optimizer.t == 3
    for _ in range(21):
        b.train(src, tar, BS, None, None)
    same_state(f, b)


# ---- the planted critic, graph = 1 -----------------------------------------------------------------------------------------------
def device_rows(seed, dev):
    from mobody_amd.algo import utils
    r = list(gu.gi.batch(seed, 64, S, A))
    rb = utils.ReplayBuffer(S, A, dev, max_size=64, rng="device", seed=seed)
    rb.convert_D4RL(dict(observations=r[0], actions=r[1], next_observations=r[2], rewards=np.full(64, 1e4, np.float32),
                         terminals=1.0 - r[4][:, 0]))
    return rb


class EnqueuedGraph:
    """Stands in for torch.cuda.CUDAGraph in the comparison run: replay() enqueues the step's closures."""
    capturing = None

    def __init__(self):
        self.closures = []

    def replay(self):
        for c in self.closures:
            c()


@contextlib.contextmanager
def enqueued_capture(g, **kw):
    EnqueuedGraph.capturing = g
    try:
        yield
    finally:
        EnqueuedGraph.capturing = None


def enqueue_instead_of_replaying(pol):
    segments = pol._graph_segments

    def deferred(*a, **k):
        def wrap(seg):
            def run():
                if EnqueuedGraph.capturing is not None:
                    EnqueuedGraph.capturing.closures.append(seg)
                else:
                    seg()
            return run
        return [wrap(s) for s in segments(*a, **k)]
    pol._graph_segments = deferred


@pytest.mark.parametrize("algo", ALGOS)
def test_fallback_with_the_graph_path_on(algo, cadence, dev, monkeypatch):
    out = {}
    for kind in ("replayed", "enqueued"):
        pol = build(algo, dev, "fallback", "f16x2", graph=1, rng="device", seed=7)
        plant_critic(pol)
        src, tar = device_rows(501, dev), device_rows(502, dev)
        if kind == "enqueued":
            monkeypatch.setattr(torch.cuda, "CUDAGraph", EnqueuedGraph)
            monkeypatch.setattr(torch.cuda, "graph", enqueued_capture)
            enqueue_instead_of_replaying(pol)
        fell, keys = [], []                                      # (call, graph key) whenever the key changes
        watch(pol, fell)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            for i in range(EVERY + 1 + 20):
                pol.train(src, tar, BS, None, None)
                assert (pol._graph is not None) == (i > 0), "every call but the first goes through the graph path"
                if not keys or keys[-1][1] != pol._graph_key:
                    keys.append((i, pol._graph_key))
                if i == 1:
                    assert pol.precision == 4                  # a graph of the f16x2 step exists before the fault
        msg, step = fault_step(rec)
        assert fell == [EVERY + 1] and "q_funcs" in msg and step == 3, "precondition: the planted weight crosses in the third step"
        # captured at precision 4 before the fault, and again at precision 3 in the call that fell back: nothing of the old graph is left
        assert keys[0] == (0, None) and keys[1][0] == 1 and all(4 in k and 3 not in k for i, k in keys[1:] if i < EVERY)
        assert any(i == EVERY for i, _ in keys) and all(3 in k and 4 not in k for i, k in keys if i >= EVERY)
        assert pol.q_optimizer.t == 3 + 21 and all(np.isfinite(x) for x in pol.losses())
        out[kind] = pol
    same_state(out["replayed"], out["enqueued"])
    assert torch.equal(out["replayed"]._ctr, out["enqueued"]._ctr)


# ---- nets beyond the critic --------------------------------------------------------------------------------------------------------
def beyond_the_critic(algo, pol):
    """(net, its name in the message, its learning rate)"""
    if algo == "iql":
        return pol.v_func, "v_func", pol.v_optimizer.lr
    if algo == "dara":
        return pol.classifier.sa_classifier, "classifier.sa_classifier", pol.classifier.opt_sa.lr
    return pol.info.encoder_sa, "info.encoder_sa", pol.info_optimizer.lr


@pytest.mark.parametrize("guard", ("raise", "fallback"))
@pytest.mark.parametrize("algo", ("iql", "dara", "igdf"))
def test_a_fault_in_a_net_beyond_the_critic_is_named_and_falls_back(algo, guard, cadence, dev):
    from mobody_amd import ops
    src, tar = rows(501, dev), rows(502, dev)
    pol = build(algo, dev, guard, "f16x2")
    net, name, lr = beyond_the_critic(algo, pol)
    plant_pairs(net, lr)
    fell = []
    watch(pol, fell)

    def run():
        if algo == "igdf":                                       # the encoders train in update_info alone: three steps, then train()
            pol.update_info(src, tar, BS, None)
            torch.cuda.synchronize()
            assert float(ops._mlp_w2(net.blob, net.layout, 1).abs().max()) >= ops.F16_W_LIMIT, "precondition: no planted weight crossed"
            pol.train(src, tar, BS, None, None)                  # total_it 1: a check point
            return
        for i in range(EVERY + 1):
            pol.train(src, tar, BS, None, None)
            if i == 0:
                torch.cuda.synchronize()
                assert float(ops._mlp_w2(net.blob, net.layout, 1).abs().max()) >= ops.F16_W_LIMIT, "precondition: no planted weight crossed"
    if guard == "raise":
        with pytest.raises(FloatingPointError, match=re.escape(name) + r" \(max \|W2\|") as ei:
            run()
        print(algo, "|", str(ei.value)[:200])
        assert "F16_RANGE" in str(ei.value) and "no policy network" not in str(ei.value) and pol.precision == 4
        return
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        run()                                                    # does not raise
    msg, _ = fault_step(rec)
    assert name + " (max |W2|" in msg and "no policy network" not in msg
    assert fell == [1 if algo == "igdf" else EVERY + 1] and pol.precision == 3 and net.precision == 3
    if algo == "igdf":
        assert pol._info_graph is None
    for _ in range(3):                                           # and goes on
        pol.train(src, tar, BS, None, None)
    if algo == "igdf":
        pol.update_info(src, tar, BS, None)
    torch.cuda.synchronize()
    assert ops.health_read(ops.health_bound(dev))[0] == 0
    assert all(bool(torch.isfinite(n.blob).all()) for n in all_nets(pol)) and all(np.isfinite(x) for x in pol.losses())


# ---- BOSA's critic / actor stage ---------------------------------------------------------------------------------------------------
BOSA_DELTA = 3.5 * LR           # the pairs cross in the critic's fourth step: both stage-2 graphs exist by then (calls 3 and 4)


def bosa_make(dev, monkeypatch, guard, mfma, graph_key, plant=True):
    """BOSA in its second stage from the first call (vae_iteration 0), rng = 'device': every draw is a function of the counts."""
    from test_hip_bosa_class import buffers, load_scaled, make
    monkeypatch.setenv("MOBODY_MFMA", mfma)
    pol = make(dev, vae_iteration=0, critic_actor=1, rng="device", seed=3, f16_guard=guard, critic_actor_graph=graph_key)
    BUILT.append(pol)
    load_scaled(pol)
    assert pol.precision == {"f16x2": 4, "bf16x3": 3}[mfma] and pol.critic_optimizer.lr == LR
    if plant:
        sd = {k: v.clone() for k, v in pol.critic.state_dict().items()}
        k1, k2 = (int(x) for x in torch.argsort(sd["network1.network.0.bias"], descending=True)[:2])
        for n in (3, 77, 150, 222):
            sd["network1.network.2.weight"][n, k1] = LIMIT - BOSA_DELTA
            sd["network1.network.2.weight"][n, k2] = -(LIMIT - BOSA_DELTA)
        pol.critic.load_state_dict(sd)
        copy_into_clone(pol.critic_target, pol.critic)
    src, tar = buffers(dev, rng="device", seed=9)
    return pol, src, tar


def bosa_nets(pol):
    return (pol.actor, pol.critic, pol.actor_target, pol.critic_target)


def bosa_run(pol, src, tar, calls):
    fell = []
    watch(pol, fell, nets=bosa_nets, opts=lambda p: (p.critic_optimizer, p.actor_optimizer), hyp=lambda p: p._hyp)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        for _ in range(calls):
            pol.train(src, tar, BS, None, None)
    torch.cuda.synchronize()
    msg, step = fault_step(rec)
    assert "critic (max |W2|" in msg and step is not None and 3 <= step < EVERY, "precondition: a planted weight crosses in steps 3 .. 7"
    assert fell == [EVERY] and pol.precision == 3 and pol._hyp.precision == 3        # the check of the ninth call (total_it 8 before it)
    return msg, step


def test_bosa_stage2_fallback_eager_and_replayed(cadence, dev, monkeypatch, tmp_path):
    from mobody_amd import ops
    from test_hip_bosa_actor import differing, nets_state
    from test_hip_bosa_graph import counts
    calls = EVERY + 1 + 20
    # the frozen state, from a 'raise' twin
    a, asrc, atar = bosa_make(dev, monkeypatch, "raise", "f16x2", 0)
    with pytest.raises(FloatingPointError, match=r"critic \(max \|W2\|") as ei:
        for _ in range(EVERY + 1):
            a.train(asrc, atar, BS, None, None)
    assert a.total_it == EVERY and "F16_RANGE" in str(ei.value)
    prefix = str(tmp_path / "frozen")
    a._save_stage2(prefix)                          # (save() itself reads the words first and reports the fault again)
    ops.health_clear()
    # the eager run under test
    f, fsrc, ftar = bosa_make(dev, monkeypatch, "fallback", "f16x2", 0)
    msg, step = bosa_run(f, fsrc, ftar, calls)
    print("bosa |", msg[:160])
    assert f.critic_optimizer.t == calls and f.total_it == calls                    # the frozen steps stay counted
    assert all(np.isfinite(x) for x in f.losses())
    # a fresh bf16x3 object with the frozen state and the same counts
    b, bsrc, btar = bosa_make(dev, monkeypatch, "raise", "bf16x3", 0, plant=False)
    b._load_stage2(lambda s: torch.load(prefix + s, map_location="cpu", weights_only=True), prefix)
    b.total_it, b._noise_calls = a.total_it, a._noise_calls
    bsrc._draws, btar._draws = asrc._draws, atar._draws
    assert b.critic_optimizer.t == EVERY
    for _ in range(21):
        b.train(bsrc, btar, BS, None, None)
    torch.cuda.synchronize()
    assert differing(nets_state(f), nets_state(b), skip=("scalars",)) == []
    assert counts(f, fsrc, ftar) == counts(b, bsrc, btar)
    for n, m in zip(bosa_nets(f), bosa_nets(b)):
        assert torch.equal(bits(n.blob_T), bits(m.blob_T))
    # the same run replayed
    g, gsrc, gtar = bosa_make(dev, monkeypatch, "fallback", "f16x2", 1)
    before = {}
    real = g._health_check

    def check():
        before.setdefault(g.total_it, (dict(g.stage2_captures), g.stage2_replays, g._s2_graph_key))
        real()
    g._health_check = check
    _, gstep = bosa_run(g, gsrc, gtar, calls)
    assert gstep == step
    caps, replays, key = before[EVERY]
    assert caps == {"critic": 1, "actor": 1} and replays == EVERY - 2 and 4 in key and 3 not in key      # both f16x2 graphs existed and ran
    assert g.stage2_captures == {"critic": 2, "actor": 2} and 3 in g._s2_graph_key and 4 not in g._s2_graph_key
    assert g.stage2_replays == calls - 2 - 3                       # eager: the first two calls and the check points 9, 17, 25
    assert differing(nets_state(g), nets_state(f), skip=("scalars",)) == [], "the replayed fallback run differs from the eager one"
    assert counts(g, gsrc, gtar) == counts(f, fsrc, ftar)
