"""Device health words through the C ABI (include/mobody_hip.h, "device health words").

The f16x2 weight planes hold w * 2^8 as two fp16 terms, so a W2 value with |w| >= 65504 / 2^8 = 255.875 is Inf in its plane.
The kernels that write weights report that -- and any non-finite optimizer result -- into a caller-owned block of device
words, and every later optimizer launch applies nothing while a bit is set.

The planted case is derived, not measured: W2 elements at 255.0 and 254.0, zero moments, step 1, |lr| = 1.  Adam's first step
is lr * g / (|g| + 1e-8), i.e. 1.0 in magnitude for |g| >> 1e-8, so the elements land at ~256.0 (>= 255.875: a fault) and
~255.0 (below it: none).  Tolerances on the fp32 results are the existing k_adam ones (test_hip_train.test_adam_polyak_kernel).
Nothing here provokes a GPU fault: Inf / NaN in a plane is ordinary arithmetic."""
import numpy as np
import pytest
import torch

import golden_util as gu
from oracle import mobody_oracle as O

pytestmark = pytest.mark.gpu

S, A, N, NT = 17, 6, 256, 192
MODES = ["f16x2", "f32", "bf16x3"]


def wide_idx(k, n):
    return ((k // 4) * 256 + n) * 4 + k % 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def words(dev):
    """A fresh health block bound for the test; unbound afterwards whatever happened."""
    from mobody_amd import ops, _lib
    w = torch.zeros(_lib.HEALTH_WORDS, dtype=torch.int32, device=dev)
    ops.health_bind(w)
    try:
        yield w
    finally:
        torch.cuda.synchronize()
        ops.health_bind(None)


def close(a, b, rtol, atol):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def same(x, y):
    """Bit-for-bit (NaN payloads and the 16-bit planes packed into float slots included)."""
    return torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y)


def mask(words):
    torch.cuda.synchronize()
    return int(words[0])


class Net:
    """Twin-Q blob with planted W2 elements, its target, T blobs and zero Adam moments."""

    def __init__(self, dev, mode, planted, seed=3, target=True):
        from mobody_amd import ops, _lib
        self.ops, self.mode = ops, mode
        self.L = L = _lib.mlp_layout(S + A, 1, 2)
        rng = np.random.default_rng(seed)
        p0 = (rng.standard_normal(L.total_floats) * 0.1).astype(np.float32)
        for (k, n), val in planted.items():
            p0[L.w2 + wide_idx(k, n)] = val
        self.p = torch.from_numpy(p0).to(dev)
        self.pT = ops.mlp_transpose(self.p, S + A, 1, 2, precision=mode)
        self.tg = self.p.clone() if target else None
        self.tgT = self.pT.clone() if target else None
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.rng = rng

    def grad(self, planted_g=None):
        g = (self.rng.standard_normal(self.L.total_floats) * 10.0 ** self.rng.uniform(-4, 0, self.L.total_floats)).astype(np.float32)
        for (k, n), val in (planted_g or {}).items():
            g[self.L.w2 + wide_idx(k, n)] = val
        return torch.from_numpy(g).to(self.p.device)

    def state(self):
        torch.cuda.synchronize()
        return [x.clone() for x in (self.p, self.pT, self.m, self.v, self.tg, self.tgT) if x is not None]


E1, E2 = (8, 5), (77, 130)          # the 255.0 and the 254.0 element


def adam(net, g, t, lr, tau, t_dev=None):
    kw = dict(target_T=net.tgT, precision=net.mode)
    if t_dev is None:
        net.ops.adam_polyak(S + A, 1, 2, net.p, net.pT, g, net.m, net.v, net.tg, t, lr, tau, **kw)
    else:
        net.ops.adam_polyak_dev(S + A, 1, 2, net.p, net.pT, g, net.m, net.v, net.tg, t_dev, lr, tau, **kw)


@pytest.mark.parametrize("form", ["host_count", "device_count"])
@pytest.mark.parametrize("mode", MODES)
def test_range_fault_adam_polyak(mode, form, dev, words):
    """255.0 -> ~256.0 under Adam: F16_RANGE in f16x2 only; fp32 results exact; the next update is frozen; clear re-arms."""
    from mobody_amd import ops, _lib
    net = Net(dev, mode, {E1: 255.0, E2: 254.0})
    t_dev = torch.ones(1, dtype=torch.int64, device=dev) if form == "device_count" else None
    g1 = net.grad({E1: -1e-2, E2: -1e-2})
    P, M, V, TG = net.p.cpu().clone(), torch.zeros(net.L.total_floats), torch.zeros(net.L.total_floats), net.tg.cpu().clone()
    adam(net, g1, 1, 1.0, 0.005, t_dev)
    O.adam_update(P, g1.cpu(), M, V, 1, 1.0)
    TG.copy_(0.005 * P + 0.995 * TG)
    got = mask(words)
    e1, e2 = net.L.w2 + wide_idx(*E1), net.L.w2 + wide_idx(*E2)
    print(f"mode {mode} form {form}: word {words.tolist()} p[e1] {float(net.p[e1])!r} p[e2] {float(net.p[e2])!r}")
    assert float(net.p[e1]) >= ops.F16_W_LIMIT > float(net.p[e2])        # the derived landing points
    assert torch.isfinite(net.p).all() and torch.isfinite(net.m).all() and torch.isfinite(net.v).all()
    close(net.p, P, rtol=2e-6, atol=1e-7); close(net.tg, TG, rtol=2e-6, atol=1e-7)
    close(net.m, M, rtol=2e-6, atol=1e-8); close(net.v, V, rtol=2e-6, atol=1e-20)
    if mode != "f16x2":
        assert got == 0
        before = net.state()
        adam(net, net.grad(), 2, 1e-3, 0.005, t_dev)
        after = net.state()
        assert mask(words) == 0 and not torch.equal(before[0], after[0])     # the second update applies
        return
    assert got == _lib.HEALTH_F16_RANGE
    assert ops.health_read(words) == (_lib.HEALTH_F16_RANGE, 1)              # the step of the faulting launch
    before = net.state()
    td0 = None if t_dev is None else t_dev.clone()
    adam(net, net.grad(), 2, 1e-3, 0.005, t_dev)                             # fresh gradients: frozen
    for x, y in zip(before, net.state()):
        assert same(x, y)
    assert t_dev is None or torch.equal(t_dev, td0)
    ops.health_clear()
    adam(net, net.grad(), 2, 1e-3, 0.005, t_dev)
    after = net.state()
    assert not torch.equal(before[0], after[0]) and not torch.equal(before[2], after[2])   # applies again
    assert mask(words) == _lib.HEALTH_F16_RANGE                              # ... and the element is still out of range


def test_range_fault_negative_control(dev, words):
    """Only the 254.0 element: ~255.0 after the step, below the bound -- the word stays 0 and updates go on."""
    net = Net(dev, "f16x2", {E2: 254.0})
    adam(net, net.grad({E2: -1e-2}), 1, 1.0, 0.005)
    assert mask(words) == 0
    before = net.state()
    adam(net, net.grad(), 2, 1e-3, 0.005)
    assert mask(words) == 0 and not torch.equal(before[0], net.state()[0])


def test_polyak_target_planes(dev, words):
    """The target's planes alone (no online T blob): tau = 1 copies the ~256.0 online value into them -> F16_RANGE;
    with the usual tau the target stays small and nothing is raised."""
    from mobody_amd import ops, _lib
    for tau, want in ((0.005, 0), (1.0, _lib.HEALTH_F16_RANGE)):
        net = Net(dev, "f16x2", {E1: 255.0})
        net.tg[net.L.w2 + wide_idx(*E1)] = 0.1
        ops.mlp_transpose(net.tg, S + A, 1, 2, out=net.tgT, precision="f16x2")
        ops.health_clear()
        ops.adam_polyak(S + A, 1, 2, net.p, None, net.grad({E1: -1e-2}), net.m, net.v, net.tg, 1, 1.0, tau, target_T=net.tgT,
                        precision="f16x2")
        got = mask(words)
        tv = float(net.tg[net.L.w2 + wide_idx(*E1)])
        print(f"tau {tau}: word {words.tolist()} target element {tv!r}")
        assert (tv >= ops.F16_W_LIMIT) == bool(want) and got == want
        before = net.state()
        ops.adam_polyak(S + A, 1, 2, net.p, None, net.grad(), net.m, net.v, net.tg, 2, 1e-3, tau, target_T=net.tgT, precision="f16x2")
        frozen = all(same(x, y) for x, y in zip(before, net.state()))
        assert frozen == bool(want)


def test_plane_builders_flag_out_of_range_weights(dev, words):
    """mobody_mlp_transpose and mobody_dyn_planes called directly (the host-side check of ops.* refuses 300.0 with a
    ValueError before it reaches them): both raise F16_RANGE in mode 4 and neither does in the bf16 format."""
    from mobody_amd import ops, _lib
    lib = _lib.load()
    L = _lib.mlp_layout(S + A, 1, 2)
    blob = torch.zeros(L.total_floats, device=dev)
    blob[L.member_floats + L.w2 + wide_idx(3, 9)] = -300.0
    bt = torch.empty(L.t_total_floats, device=dev)
    D = _lib.dyn_layout(S, A)
    dblob = torch.zeros(D.total_floats, device=dev)
    y = D.layer[_lib.DL_NAMES.index("transition2")]
    dblob[y.w_off + 2 * y.Kp * y.Np + wide_idx(200, 17)] = 300.0
    planes = torch.empty(lib.mobody_dyn_planes_floats(), device=dev)
    for prec, want in ((3, 0), (4, _lib.HEALTH_F16_RANGE)):
        ops.health_clear()
        _lib.check(lib.mobody_mlp_transpose(S + A, 1, 2, _lib.ptr(blob), _lib.ptr(bt), prec, _lib.cur_stream()))
        assert mask(words) == want
        ops.health_clear()
        _lib.check(lib.mobody_dyn_planes(_lib.ptr(dblob), S, A, _lib.ptr(planes), prec, _lib.cur_stream()))
        assert mask(words) == want
    ops.health_clear()
    blob[L.member_floats + L.w2 + wide_idx(3, 9)] = 255.0            # in range: silent
    _lib.check(lib.mobody_mlp_transpose(S + A, 1, 2, _lib.ptr(blob), _lib.ptr(bt), 4, _lib.cur_stream()))
    assert mask(words) == 0


def test_nonfinite_update_is_flagged_and_freezes(mfma, dev, words):
    """One NaN gradient entry -> NONFINITE in every mode; later updates are frozen."""
    from mobody_amd import ops, _lib
    net = Net(dev, mfma, {})
    g = net.grad()
    g[net.L.b2 + 7] = float("nan")                                   # a bias entry: no plane involved
    adam(net, g, 1, 3e-4, 0.005)
    assert mask(words) == _lib.HEALTH_NONFINITE
    assert torch.isnan(net.p[net.L.b2 + 7]) and int(torch.isnan(net.p).sum()) == 1
    before = net.state()
    adam(net, net.grad(), 2, 3e-4, 0.005)
    for x, y in zip(before, net.state()):
        assert same(x, y)


# ------------------------------------------------------------------------------------------------ the whole step
def _engine(dev, seed=31):
    from mobody_amd.engine import Engine
    pa, pq, _ = gu.policy_params(seed, S, A)
    return Engine(S, A, pa, pq, dev)


def _batch(dev, seed):
    return [torch.as_tensor(x, dtype=torch.float32).to(dev).contiguous() for x in gu.gi.batch(seed, N, S, A)]


def _fused_step(e, cfg, b, ws, t=None, c=None, lr_q=None):
    """critic update -> actor forward -> actor update; host step count t, or the device words c = [bump, t_q, t_pi]."""
    ops = e.ops
    dims, hyp = ops.train_dims(S, A, N, NT), ops.hyper(cfg)
    lr_q = cfg["critic_lr"] if lr_q is None else lr_q
    kq = dict(t_dev=c[1:2], bump=c[0:1]) if c is not None else {}
    ka = dict(t_dev=c[2:3]) if c is not None else {}
    if c is not None:
        ops.counter_add(c[1:3])
    ops.critic_update(dims, hyp, e.actor, e.q, e.q_T, e.qt, b, e.mq, e.vq, t or 0, lr_q, e.loss[0:1], ws,
                      actor_blob_T=e.actor_T, qtarg_blob_T=e.qt_T, **kq)
    ops.actor_forward(dims, hyp, e.actor, e.q, b[0], b[1], e.stats, ws, actor_blob_T=e.actor_T, q_blob_T=e.q_T)
    ops.actor_update(dims, hyp, e.actor, e.actor_T, e.q, e.q_T, b[0], b[1], e.stats, e.ma, e.va, t or 0, cfg["actor_lr"],
                     e.loss[1:3], ws, **ka)


NAMES = ("q", "q_T", "qt", "qt_T", "mq", "vq", "actor", "actor_T", "ma", "va", "loss")


def _snap(e):
    torch.cuda.synchronize()
    return {k: getattr(e, k).clone() for k in NAMES}


@pytest.mark.parametrize("tag", ["default", "noqw", "bc05"])
@pytest.mark.parametrize("replay", [False, True])
def test_bound_word_changes_nothing(tag, replay, mfma, dev):
    """Two steps of a G7 variant with the word bound and with none bound: parameters, moments, losses and T blobs are
    bit-identical and the word stays 0 -- eagerly and as a captured graph (bound before the capture)."""
    from mobody_amd import ops, _lib
    cfg = gu.policy_cfg(S, A, mfma=mfma, **gu.G7_VARIANTS[tag])
    b = _batch(dev, 8)
    ws = ops.train_workspace(ops.train_dims(S, A, N, NT), dev)
    outs = []
    w = torch.zeros(_lib.HEALTH_WORDS, dtype=torch.int32, device=dev)
    try:
        for bound in (False, True):
            ops.health_bind(w if bound else None)
            e = _engine(dev)
            snaps = []
            if replay:
                c = torch.zeros(3, dtype=torch.int64, device=dev)
                _fused_step(e, cfg, b, ws, c=c)                       # warm-up outside the capture, then start over
                torch.cuda.synchronize()
                e, c = _engine(dev), torch.zeros(3, dtype=torch.int64, device=dev)
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    _fused_step(e, cfg, b, ws, c=c)
                for _ in (1, 2):
                    gr.replay()
                    snaps.append(_snap(e))
                assert c.tolist() == [2, 2, 2]
            else:
                for t in (1, 2):
                    _fused_step(e, cfg, b, ws, t=t)
                    snaps.append(_snap(e))
            outs.append(snaps)
        assert w.tolist() == [0] * _lib.HEALTH_WORDS
    finally:
        torch.cuda.synchronize()
        ops.health_bind(None)
    for s0, s1 in zip(*outs):
        for k in NAMES:
            assert same(s0[k], s1[k]), k
    assert not torch.equal(outs[0][0]["q"], outs[0][1]["q"])


def _plant_critic(dev, cfg, b, ws):
    """An engine whose critic has W2[k1][n] = 255.0 and W2[k2][n] = 254.0 (member 0, online and target) at a place where the
    batch's gradient has one sign on both, and the learning rate of magnitude 1 that moves them outwards."""
    from mobody_amd import ops, _lib
    L = _lib.mlp_layout(S + A, 1, 2)
    dims, hyp = ops.train_dims(S, A, N, NT), ops.hyper(cfg)
    for n in (5, 40, 99, 130, 201, 250):
        for k1, k2 in ((8, 77), (20, 141), (66, 3), (190, 35)):
            e = _engine(dev)
            e.q[L.w2 + wide_idx(k1, n)] = 255.0
            e.q[L.w2 + wide_idx(k2, n)] = 254.0
            e.qt.copy_(e.q)
            ops.mlp_transpose(e.q, S + A, 1, 2, out=e.q_T, precision=e.prec)
            e.qt_T.copy_(e.q_T)
            ops.critic_step(dims, hyp, e.actor, e.q, e.q_T, e.qt, b, e.gq, e.loss[0:1], ws, actor_blob_T=e.actor_T,
                            qtarg_blob_T=e.qt_T)
            torch.cuda.synchronize()
            g1, g2 = float(e.gq[L.w2 + wide_idx(k1, n)]), float(e.gq[L.w2 + wide_idx(k2, n)])
            if g1 * g2 > 0 and min(abs(g1), abs(g2)) > 1e-6 and bool(torch.isfinite(e.gq).all()):
                return e, L.w2 + wide_idx(k1, n), L.w2 + wide_idx(k2, n), (1.0 if g1 < 0 else -1.0)
    raise AssertionError("no planted pair with a common gradient sign among the candidates")


@pytest.mark.parametrize("mode", MODES)
def test_range_fault_fused_critic_update(mode, dev, words):
    """The same planted case through mobody_critic_update (the gradient is the batch's; lr = +-1 moves both elements out)."""
    from mobody_amd import ops, _lib
    cfg = gu.policy_cfg(S, A, mfma=mode)
    b, b2 = _batch(dev, 8), _batch(dev, 9)
    dims, hyp = ops.train_dims(S, A, N, NT), ops.hyper(cfg)
    ws = ops.train_workspace(dims, dev)
    import os
    os.environ["MOBODY_MFMA"] = mode                                     # Engine builds its T blobs in the default mode
    try:
        e, e1, e2, lr = _plant_critic(dev, cfg, b, ws)
    finally:
        os.environ.pop("MOBODY_MFMA", None)
    P, M, V, TG = e.q.cpu().clone(), torch.zeros_like(e.q).cpu(), torch.zeros_like(e.q).cpu(), e.qt.cpu().clone()
    O.adam_update(P, e.gq.cpu(), M, V, 1, lr)                            # the gradient of the very same state (critic_step)
    TG.copy_(cfg["tau"] * P + (1.0 - cfg["tau"]) * TG)
    bump = torch.zeros(1, dtype=torch.int64, device=dev)
    upd = lambda batch, t, rate: ops.critic_update(dims, hyp, e.actor, e.q, e.q_T, e.qt, batch, e.mq, e.vq, t, rate, e.loss[0:1],
                                                   ws, actor_blob_T=e.actor_T, qtarg_blob_T=e.qt_T, bump=bump)
    assert mask(words) == 0
    upd(b, 1, lr)
    got = mask(words)
    print(f"mode {mode}: lr {lr} word {words.tolist()} q[e1] {float(e.q[e1])!r} q[e2] {float(e.q[e2])!r}")
    assert float(e.q[e1]) >= ops.F16_W_LIMIT > float(e.q[e2])
    assert all(bool(torch.isfinite(x).all()) for x in (e.q, e.mq, e.vq, e.qt))
    close(e.q, P, rtol=2e-6, atol=1e-7); close(e.qt, TG, rtol=2e-6, atol=1e-7)
    close(e.mq, M, rtol=2e-6, atol=1e-8); close(e.vq, V, rtol=2e-6, atol=1e-20)
    assert int(bump) == 1
    st = lambda: [x.clone() for x in (e.q, e.q_T, e.qt, e.qt_T, e.mq, e.vq, bump)]
    before = st()
    upd(b2, 2, 1e-3)
    torch.cuda.synchronize()
    if mode != "f16x2":
        assert got == 0 and mask(words) == 0
        assert not torch.equal(before[0], e.q) and int(bump) == 2
        return
    assert got == _lib.HEALTH_F16_RANGE
    for x, y in zip(before, st()):
        assert same(x, y)
    ops.health_clear()
    upd(b2, 2, 1e-3)
    torch.cuda.synchronize()
    assert not torch.equal(before[4], e.mq) and int(bump) == 2            # applies again
    assert mask(words) != 0                                              # (from planes that hold Inf: flagged again)


def test_graph_replay_freezes_at_the_faulting_step(dev, words):
    """The captured steady-state step, a planted 255.0 critic weight and a learning rate that crosses the bound in the first
    replay.  Ten replays later the bit is set, everything is finite and the state is the one after the faulting launch alone:
    the critic's update of replay 1 applied, the actor's update of that replay (first launch after the fault) and all of
    replays 2-10 did not."""
    from mobody_amd import ops, _lib
    import os
    cfg = gu.policy_cfg(S, A, mfma="f16x2")
    b = _batch(dev, 8)
    dims, hyp = ops.train_dims(S, A, N, NT), ops.hyper(cfg)
    ws = ops.train_workspace(dims, dev)
    os.environ["MOBODY_MFMA"] = "f16x2"
    try:
        e, e1, e2, lr = _plant_critic(dev, cfg, b, ws)
        ref = _engine(dev)
    finally:
        os.environ.pop("MOBODY_MFMA", None)
    for k in ("q", "q_T", "qt", "qt_T"):
        getattr(ref, k).copy_(getattr(e, k))
    _fused_step(_engine(dev), cfg, b, ws, c=torch.zeros(3, dtype=torch.int64, device=dev))   # every kernel has run once before the capture
    torch.cuda.synchronize()
    assert int(words[0]) == 0
    # reference: the critic update alone, with no word bound (device step count, as in the graph)
    ops.health_bind(None)
    cr = torch.tensor([0, 1, 1], dtype=torch.int64, device=dev)
    ops.critic_update(dims, hyp, ref.actor, ref.q, ref.q_T, ref.qt, b, ref.mq, ref.vq, 0, lr, ref.loss[0:1], ws,
                      actor_blob_T=ref.actor_T, qtarg_blob_T=ref.qt_T, t_dev=cr[1:2], bump=cr[0:1])
    torch.cuda.synchronize()
    ops.health_bind(words)
    c = torch.zeros(3, dtype=torch.int64, device=dev)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):                                           # (captured kernels do not run: the state is untouched)
        _fused_step(e, cfg, b, ws, c=c, lr_q=lr)
    for _ in range(10):
        gr.replay()
    torch.cuda.synchronize()
    print(f"word {words.tolist()} counters {c.tolist()} q[e1] {float(e.q[e1])!r} q[e2] {float(e.q[e2])!r}")
    assert int(words[0]) == _lib.HEALTH_F16_RANGE and int(words[1]) == 1
    assert float(e.q[e1]) >= ops.F16_W_LIMIT > float(e.q[e2])
    for k in ("q", "qt", "mq", "vq", "actor", "ma", "va"):
        assert bool(torch.isfinite(getattr(e, k)).all()), k
    for k in ("q", "q_T", "qt", "qt_T", "mq", "vq", "actor", "actor_T", "ma", "va"):
        assert same(getattr(e, k), getattr(ref, k)), k
    assert int(c[0]) == 1                                                # `bump` advanced once, by the faulting launch
