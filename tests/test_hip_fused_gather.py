"""The minibatch gather inside the critic's first forward launch (MobodyCritic.gather, config['fused_gather']).

Everything here is bit-for-bit against the unfused path of the same build -- mobody_gather_batch_rng followed by
mobody_critic_update: the two perform the same draws, the same loads and the same arithmetic, so there is no tolerance."""
import functools
import types

import pytest
import torch

import golden_util as gu
from mobody_amd import _lib, ops

SHAPES = [(17, 6), (11, 3), (111, 8)]            # (111, 8): a tile's part of the ring row is more than 16 chunks per lane group
COUNTS = [(33, 31, 17),                          # partial last tile; tiles that straddle both buffer boundaries
          (32, 32, 0),                           # no fake buffer; boundaries on tile edges
          (256, 256, 128),
          (1, 1, 1)]
RING_ROWS = (100000, 5, 300)                     # src | tar | fake: 31 rows are drawn from the 5-row ring
PAD = 5                                          # sentinel rows behind the minibatch arrays


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _rings(S, A):
    """Three packed rings of RING_ROWS rows with every float (padding included) random, and their {ptr, size} words."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(1000 * S + A)
    pitch = ops.ring_pitch(S, A)
    out = []
    for rows in RING_ROWS:
        store = torch.randn(rows, pitch, generator=g).to(dev)
        out.append((ops.RingView(store, S, A), torch.tensor([0, rows], dtype=torch.int64, device=dev)))
    return out


@functools.lru_cache(maxsize=None)
def _nets(S, A, mfma):
    from mobody_amd import engine
    pa, pq, _ = gu.policy_params(5, S, A)
    return engine.Engine(S, A, pa, pq, torch.device("cuda:0"))        # built under MOBODY_MFMA = mfma (the fixture set it)


def _critic_call(S, A, mfma, counts, fused, views=None, q_next=None, phase=0):
    """One critic update from a fixed state; returns every tensor it can have written."""
    dev = torch.device("cuda:0")
    eng = _nets(S, A, mfma)
    cfg = gu.policy_cfg(S, A, mfma=mfma)
    rings = _rings(S, A)[:len([c for c in counts if c > 0])]
    counts = [c for c in counts if c > 0]
    N, Nt = sum(counts), counts[0] + counts[1]
    dims, hyp = ops.train_dims(S, A, N, Nt), ops.hyper(cfg)
    nan = float("nan")
    full = [torch.full((N + PAD, w), nan, device=dev) for w in (S, A, S, 1, 1)]
    b = tuple(t[:N] for t in full)
    ws = ops.train_workspace(dims, dev)
    _bits(ws).fill_(-1)                                               # 0xFF bytes: xq, q, pin, sign words, h1 planes, ...
    st = {k: getattr(eng, k).clone() for k in ("actor", "actor_T", "q", "q_T", "qt", "qt_T", "mq", "vq")}
    loss = torch.zeros(1, device=dev)
    ctr = torch.tensor([7, 3, 11, 13], dtype=torch.int64, device=dev)  # call counter | the three words the gather advances
    gather = dict(buffers=views if views is not None else [r[0] for r in rings], counts=counts, seeds=[101, 102, 103][:len(counts)],
                  call_offsets=[1] * len(counts), counter=ctr[0:1], sizes=[r[1][1:2] for r in rings], bump=(ctr[1:2], ctr[2:3], ctr[3:4]))
    kw = dict(t_dev=ctr[1:2], policy_forward=True, actor_blob_T=st["actor_T"], qtarg_blob_T=st["qt_T"], bump=ctr[0:1],
              q_next=q_next, phase=phase)
    if fused:
        kw["gather"] = gather
    else:
        ops.gather_batch_rng(S=S, A=A, out=b, **gather)
    ops.critic_update(dims, hyp, st["actor"], st["q"], st["q_T"], st["qt"], b, st["mq"], st["vq"], 0, cfg["critic_lr"], loss, ws, **kw)
    torch.cuda.synchronize()
    out = dict(st, ws=ws, loss=loss, ctr=ctr)
    out.update({"batch%d" % k: t for k, t in enumerate(full)})
    return out, N


@pytest.mark.gpu
@pytest.mark.parametrize("S,A", SHAPES)
def test_launch_bitwise(mfma, S, A):
    for counts in COUNTS:
        ref, N = _critic_call(S, A, mfma, counts, fused=False)
        got, _ = _critic_call(S, A, mfma, counts, fused=True)
        for k in ref:
            assert torch.equal(_bits(ref[k]), _bits(got[k])), (counts, k)
        for k in range(5):
            t = got["batch%d" % k]
            assert not torch.isnan(t[:N]).any(), (counts, k)          # every row written ...
            assert (_bits(t[N:]) == _bits(torch.full_like(t[N:], float("nan")))).all(), (counts, k)   # ... and none past them
        assert got["ctr"].tolist() == [8, 4, 12, 14]                  # the optimizer launch advanced [0], the gather the rest


def _policy(S, A, graph, fused_gather):
    from mobody_amd import synthetic
    from mobody_amd.algo import utils
    from mobody_amd.algo.call_algo import call_algo
    dev, task = torch.device("cuda:0"), "walker2d-medium-v2"
    torch.manual_seed(3)
    cfg = gu.policy_cfg(S, A, rng="device", seed=7, graph=graph, src_rollout_length=0, trg_rollout_length=0,
                        use_src_sa_to_get_target_next_state=0, fused_gather=fused_gather)
    pol = call_algo("mobody", cfg, 3, dev)
    rows = gu.gi.batch(9, 300, S, A)
    pol.fake_replay_buffer.add_batch(dict(obss=rows[0], actions=rows[1], next_obss=rows[2], rewards=rows[3], terminals=1.0 - rows[4]))
    src = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=4000, rng="device", seed=1), 4000, task, 0)
    tar = synthetic.fill_buffer(utils.ReplayBuffer(S, A, dev, max_size=500, rng="device", seed=2), 500, task, 1)
    return pol, src, tar


def _state(pol):
    torch.cuda.synchronize()
    ts = [pol.q_funcs.blob, pol.target_q_funcs.blob, pol.policy.blob, pol.q_optimizer.m, pol.q_optimizer.v,
          pol.policy_optimizer.m, pol.policy_optimizer.v, pol._loss[:3], pol._ctr]
    return [t.clone() for t in ts]


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [1, 0])
def test_step_bitwise(mfma, graph, monkeypatch):
    """Six train() calls at batch 64 (the first eager, the rest replayed when graph = 1): nets, moments, losses and counters."""
    S, A = 17, 6
    taken = []
    real = ops.critic_update
    monkeypatch.setattr(ops, "critic_update", lambda *a, **k: (taken.append(k.get("gather") is not None), real(*a, **k))[1])
    fused = _policy(S, A, graph, 1)
    plain = _policy(S, A, graph, 0)
    for call in range(6):
        states = []
        for pol, src, tar in (fused, plain):
            del taken[:]
            pol.train(src, tar, 64, None, None)
            states.append((_state(pol), any(taken)))
        (sf, used_f), (sp, used_p) = states
        for k, (x, y) in enumerate(zip(sf, sp)):
            assert torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y), (call, k)
        assert not used_p
        assert used_f == (graph == 1 and call == 1)                   # the capture of the second call is where the entry is chosen
    assert fused[0].q_optimizer.t == plain[0].q_optimizer.t


@pytest.mark.gpu
def test_refusals(mfma):
    S, A = 17, 6
    counts = (33, 31, 17)
    dev = torch.device("cuda:0")
    loose = [tuple(f.contiguous() for f in r[0].fields()) for r in _rings(S, A)]      # five separate arrays per source
    with pytest.raises(_lib.MobodyError, match="row-interleaved"):
        _critic_call(S, A, mfma, counts, fused=True, views=loose)
    with pytest.raises(_lib.MobodyError, match="q_next"):
        _critic_call(S, A, mfma, counts, fused=True, q_next=torch.zeros(sum(counts), device=dev))
    for phase in (1, 2):
        with pytest.raises(_lib.MobodyError, match="phase"):
            _critic_call(S, A, mfma, counts, fused=True, phase=phase)
    torch.cuda.synchronize()                                          # refused on the host: nothing was launched, nothing faulted


# ---- which entry the captured step takes (no GPU: the library is a recorder) ----
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            gathers = name == "mobody_critic" and bool(args[0]._obj.gather)      # args[0]: byref(MobodyCritic)
            self.calls.append(name + ("+gather" if gathers else ""))
            return 0
        return fn


def _mock_step(monkeypatch, **over):
    from mobody_amd.algo.offline_offline import mobody as M
    S, A, bs = 17, 6, 64
    lib = _Recorder()
    monkeypatch.setattr(ops, "load", lambda: lib)
    monkeypatch.setattr(ops, "cur_stream", lambda: None)
    cfg = gu.policy_cfg(S, A, rng="device", mfma="f32", par_overlap=0, **over)
    pitch = (2 * S + A + 2 + 15) // 16 * 16
    z = lambda *s: torch.zeros(*s)
    ring = lambda: types.SimpleNamespace(_fields=lambda v=ops.RingView(z(8, pitch), S, A): v, ptr_size=torch.zeros(2, dtype=torch.int64))
    net = lambda: types.SimpleNamespace(blob=z(4), blob_T=z(4))
    opt = lambda: types.SimpleNamespace(m=z(4), v=z(4), t=0, lr=3e-4, step_dev=lambda *a, **k: None)
    pol = object.__new__(M.MOBODY)
    pol.config, pol.S, pol.A, pol.rng, pol.penalty_type = cfg, S, A, "device", cfg["penalty_type"]
    pol.fused_update, pol.dp_graph, pol._side_stream = 1, "captured", None
    pol._ctr = torch.zeros(4, dtype=torch.int64)
    N = int(2.5 * bs)
    pol._batch = (z(N, S), z(N, A), z(N, S), z(N, 1), z(N, 1))
    pol._seed_for = lambda k: k
    pol.fake_replay_buffer = ring()
    pol.policy, pol.q_funcs, pol.target_q_funcs, pol.v_func = net(), net(), net(), net()
    pol.q_optimizer, pol.policy_optimizer, pol.v_optimizer = opt(), opt(), opt()
    pol._loss, pol._ws = z(4), z(4)
    pol._dims = lambda N, Nt, Ng, Ntg: (ops.train_dims(S, A, N, Nt, Ng, Ntg), ops.hyper(cfg))
    pol.actor_stats = pol.actor_update = pol.value_grad = lambda *a, **k: None
    pol.dynamics = types.SimpleNamespace(step_device=lambda *a, **k: {"next_obs": z(bs, S)})
    monkeypatch.setattr(ops, "mlp3_forward", lambda *a, **k: z(N, 1))
    (step,) = pol._graph_segments(ring(), ring(), bs, 1, False)
    step()
    return [c for c in lib.calls if c.startswith(("mobody_gather", "mobody_critic"))]


def test_fused_step_takes_the_gathering_entry(monkeypatch):
    assert _mock_step(monkeypatch) == ["mobody_critic+gather"]


@pytest.mark.parametrize("over", [dict(penalty_type="par"), dict(advantage=1), dict(penalty_type="dara"), dict(fused_gather=0)],
                         ids=["par", "advantage", "dara", "off"])
def test_fused_step_falls_back_to_two_calls(monkeypatch, over):
    assert _mock_step(monkeypatch, **over) == ["mobody_gather_batch_rng", "mobody_critic"]
