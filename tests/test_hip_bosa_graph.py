"""GPU checks of BOSA's critic / actor stage without a torch op and of its replay.

mobody_bosa_target against today's composition -- mobody_rng_normal on stream 10, torch's mul / clamp / add / clamp, the two
forwards, torch.min -- BIT FOR BIT, and next to that against the fp64 restatement (tests/bosa_graph_cases.py) at rtol 1e-5 / atol 1e-5 x
max |q_next|; its clamps at planted edges, exactly; a NaN row kept to itself.  mobody_bosa_stage2_rows against torch's single
multiplies, bit for bit; mobody_bosa_stage2_words against the restatement at rtol 1e-5 / atol 1e-5 x the largest term of each word
(the bounds tests/test_hip_bosa_actor.py holds these scalars to; tests/test_bosa_graph_ref.py shows a float32 evaluation within half of
them), the copied words exactly.  The class with config['critic_actor_graph'] = 1 against the same run with 0: nets, moments and
counts bit for bit, the logged words within the scalar bounds.  Workspaces are NaN-filled with guard words behind them.

Shapes are the smallest at which these kernels can go wrong (GC.TARGET_ROWS, GC.WORDS_ROWS): one and two rows short of and past a
workgroup, and 1025 rows, where the 4 x 256-thread grid-stride loops take their second trip."""
import json
import os

import numpy as np
import pytest
import torch

import bosa_actor_cases as BC
import bosa_graph_cases as GC
from test_hip_bosa import GUARD, NAN, guard_intact
from test_hip_bosa_actor import differing, nets_state
from test_hip_bosa_class import buffers, config_tree, load_scaled, make

pytestmark = pytest.mark.gpu
STREAM = 10                                     # MOBODY_BOSA_STREAM_TARGET_NOISE


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


T = lambda p: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in p.items()}


class Target:
    """The target actor and twin-Q of a shape on the device (fixed seeds), and mobody_bosa_target calls on guarded buffers."""

    def __init__(self, S, A, dev, mode="f32", ma=1.0, actor=None):
        from mobody_amd import ops
        from mobody_amd.algo.offline_offline.mobody import _PackedNet
        prec = ops.prec_id(mode)
        self.pa, self.pq = actor if actor is not None else GC.mlp_params(5, S, A, 1), GC.mlp_params(6, S + A, 1, 2)
        self.actor = _PackedNet(S, A, 1, ("",), dev, out_mode=1, max_action=ma, init=False, precision=prec)
        self.actor.load_state_dict(T(GC.state_dict(self.pa, ("",))))
        self.critic = _PackedNet(S + A, 1, 2, ("network1.", "network2."), dev, init=False, precision=prec)
        self.critic.load_state_dict(T(GC.state_dict(self.pq, ("network1.", "network2."))))
        self.S, self.A, self.ma, self.dev = S, A, ma, dev

    def run(self, s2, noise=None, expl=GC.EXPL, clip=GC.CLIP, seed=0, call=0, call_dev=None):
        """(q_next [N], a' [N, A] as the workspace holds it)."""
        from mobody_amd import ops
        N, A = s2.shape[0], self.A
        qbuf = torch.full((N + 1,), NAN, device=self.dev)
        blk = ops.bosa_target_block(self.actor, self.critic, s2, qbuf[:-1], expl, clip, noise=noise, seed=seed, call=call, call_dev=call_dev)
        words = ops.bosa_target_workspace(blk, self.dev).numel()
        assert words == GC.target_workspace_floats(self.S, A, N)
        buf = torch.full((words + GUARD,), NAN, device=self.dev)
        blk.workspace = buf.data_ptr()
        ops.bosa_target(blk)
        torch.cuda.synchronize()
        assert guard_intact(buf) and bool(torch.isnan(qbuf[-1])), "mobody_bosa_target wrote behind a buffer"
        return qbuf[:-1].clone(), buf[:N * A].reshape(N, A).clone()

    def composition(self, s2, noise, expl=GC.EXPL, clip=GC.CLIP):
        """What critic_actor_train does with torch ops."""
        from mobody_amd import ops
        qt, N = self.critic, s2.shape[0]
        a2 = (self.actor(s2) + (noise * expl).clamp(-clip, clip)).clamp(-self.ma, self.ma)
        q = ops.mlp3_forward(qt.blob, self.S + self.A, 1, 2, s2, a2, blob_T=qt.blob_T, precision=qt.precision).min(0)[0].reshape(N).contiguous()
        torch.cuda.synchronize()
        return q, a2


def check_target(S, A, N, dev, mode, ma, vs_fp64=False):
    from mobody_amd import ops
    k = Target(S, A, dev, mode, ma)
    s2n, noisen = GC.target_inputs(S, A, N)
    s2, noise = torch.from_numpy(s2n).to(dev), torch.from_numpy(noisen).to(dev)
    want, a_want = k.composition(s2, noise)
    got, a_got = k.run(s2, noise)
    assert bits_equal(got, want) and bits_equal(a_got, a_want), ("noise given", S, A, N, mode, ma)
    assert bool(torch.isfinite(want).all()) and float(want.abs().max()) > 0
    seed = 77
    drawn = {c: ops.rng_normal(seed, STREAM, c, N * A, dev).reshape(N, A) for c in (3, 12)}
    assert not bits_equal(drawn[3], drawn[12])
    for c, d in drawn.items():                                        # noise == NULL at two calls: the stream's own draws
        w, aw = k.composition(s2, d)
        g, ag = k.run(s2, None, seed=seed, call=c)
        assert bits_equal(g, w) and bits_equal(ag, aw), ("noise drawn", S, A, N, mode, ma, c)
    word = lambda v: torch.tensor([v], dtype=torch.int64, device=dev)
    g0, _ = k.run(s2, None, seed=seed, call=12, call_dev=word(0))
    g5, _ = k.run(s2, None, seed=seed, call=7, call_dev=word(5))
    w12, _ = k.composition(s2, drawn[12])
    assert bits_equal(g0, w12) and bits_equal(g5, w12), "call = 7, call_dev = [5] is call = 12"
    if vs_fp64:
        q64, _ = GC.target_value(k.pa, k.pq, s2n, noisen, GC.EXPL, GC.CLIP, ma)
        tol = GC.RTOL * np.abs(q64) + GC.ATOL * np.abs(q64).max()
        ratio = float((np.abs(got.cpu().numpy() - q64) / tol).max())
        print("target (S, A, N) = (%d, %d, %d) ma %g: q_next vs fp64, worst error / tolerance %.4f" % (S, A, N, ma, ratio))
        assert ratio <= 1.0


# ---- 1. the bootstrap value ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,A", GC.TARGET_SHAPES)
def test_target_has_the_bits_of_the_torch_composition(S, A, dev):
    for N in GC.TARGET_ROWS:
        for ma in (1.0, 2.0):
            check_target(S, A, N, dev, "f32", ma, vs_fp64=ma == 1.0)


@pytest.mark.parametrize("mode", ("f16x2", "bf16x3"))
def test_target_has_the_bits_of_the_torch_composition_in_the_split_modes(mode, dev):
    for N in GC.SPLIT_ROWS:
        check_target(17, 6, N, dev, mode, 1.0)


@pytest.mark.parametrize("mode", ("bf16", "bf16x2"))
def test_target_refuses_the_lower_modes_by_name(mode, dev):
    from mobody_amd import _lib
    k = Target(17, 6, dev, mode)
    s2 = torch.zeros(8, 17, device=dev)
    with pytest.raises(_lib.MobodyError, match=r"mobody_bosa_target: precision \d: must be one of 0 \(f32\), 3 \(bf16x3\), 4 \(f16x2\)"):
        k.run(s2, torch.zeros(8, 6, device=dev))


def sign_actor(S, A):
    """An actor whose pre-tanh output is s[0] in every column: at s[0] = +-100 its output is +-max_action exactly."""
    z = lambda *s: np.zeros(s, np.float32)
    W1, W2, W3 = z(256, S), z(256, 256), z(A, 256)
    W1[0, 0], W1[1, 0] = 1, -1
    W2[0, 0] = W2[1, 1] = 1
    W3[:, 0], W3[:, 1] = 1, -1
    return [[W1, z(256), W2, z(256), W3, z(A)]]


@pytest.mark.parametrize("ma", (1.0, 2.0))
def test_target_action_at_the_clamp_edges_is_exact(ma, dev):
    S, A = 17, 6
    noisen, sign = GC.clamp_edge_inputs(A)
    N = len(sign)
    s2n = np.random.default_rng(4).standard_normal((N, S)).astype(np.float32)
    s2n[:, 0] = 100 * sign
    k = Target(S, A, dev, "f32", ma, actor=sign_actor(S, A))
    s2, noise = torch.from_numpy(s2n).to(dev), torch.from_numpy(noisen).to(dev)
    pi = k.actor(s2)
    torch.cuda.synchronize()
    assert np.array_equal(pi.cpu().numpy(), (sign * np.float32(ma))[:, None].repeat(A, 1)), "the planted actor sits at +-max_action"
    got, a_got = k.run(s2, noise, expl=GC.EDGE_EXPL)
    a64 = GC.target_action(pi.cpu().numpy(), noisen, GC.EDGE_EXPL, GC.CLIP, ma)
    assert np.array_equal(a_got.cpu().numpy().astype(np.float64), a64), "a' differs from the restatement, which is exact here"
    assert (a64.max(), a64.min()) == (ma, -ma) and (np.abs(a64) < ma).any()
    want, a_want = k.composition(s2, noise, expl=GC.EDGE_EXPL)
    assert bits_equal(got, want) and bits_equal(a_got, a_want)


def test_target_keeps_a_nan_row_to_itself(dev):
    S, A, N, row = 17, 6, 33, 7
    k = Target(S, A, dev)
    s2n, noisen = GC.target_inputs(S, A, N)
    s2, noise = torch.from_numpy(s2n).to(dev), torch.from_numpy(noisen).to(dev)
    clean, _ = k.run(s2, noise)
    assert bool(torch.isfinite(clean).all())
    s2[row, 3] = NAN
    got, _ = k.run(s2, noise)                          # asserts the guard words
    keep = torch.arange(N, device=dev) != row
    assert bool(torch.isnan(got[row])) and bits_equal(got[keep], clean[keep])
    noise[2, 1] = NAN                                  # and a NaN in the noise goes through both clamps
    got, a2 = k.run(s2, noise)
    assert bool(torch.isnan(a2[2, 1])) and bool(torch.isnan(got[2])) and int(torch.isnan(got).sum()) == 2


# ---- 2. the row-wise pieces and the words -------------------------------------------------------------------------------------------
def run_words(N, dev, ll=None, bump=None):
    from mobody_amd import ops
    mask, closs, ll0, aloss, dll = GC.words_inputs(N)
    ll = ll0 if ll is None else ll
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t_mask, t_closs, t_ll, t_aloss, t_dll = d(mask), d(closs), d(ll), d(aloss), d(dll)
    mm = t_mask.mean(0, keepdim=True)
    out = torch.full((N + N * 6 + 9 + GUARD,), NAN, device=dev)        # row_weight | dpi | words, one NaN, guard
    rw, dpi, words = out[:N], out[N:7 * N].reshape(N, 6), out[7 * N:7 * N + 8]
    scale = -GC.LAMDA / N
    ops.bosa_stage2_rows(N, mask=t_mask, row_weight=rw)
    ops.bosa_stage2_rows(N, dll=t_dll, dpi=dpi, dpi_scale=scale, A=6)
    kw = dict(bump=bump, bump_inc=(3, 1, 1, 1)) if bump is not None else {}
    ops.bosa_stage2_words(N, words, mask_mean=mm, closs=t_closs, cons_coef=GC.CONS, ll=t_ll, aloss=t_aloss, lamda=GC.LAMDA, **kw)
    torch.cuda.synchronize()
    assert guard_intact(out) and bool(torch.isnan(out[7 * N + 8])) and bool(torch.isnan(words[7])), "words[7] is the class's, not the kernel's"
    assert bits_equal(rw, t_mask * 0.5) and bits_equal(dpi, t_dll * scale), "row_weight / dpi are torch's single multiplies"
    both = torch.full((7 * N,), NAN, device=dev)                       # the two parts in ONE launch
    ops.bosa_stage2_rows(N, mask=t_mask, row_weight=both[:N], dll=t_dll, dpi=both[N:], dpi_scale=scale, A=6)
    torch.cuda.synchronize()
    assert bits_equal(both, out[:7 * N])
    return words[:7].cpu().numpy(), (mask, closs, ll, aloss), float(mm)


@pytest.mark.parametrize("N", GC.WORDS_ROWS)
def test_stage2_rows_and_words(N, dev):
    got, (mask, closs, ll, aloss), mm = run_words(N, dev)
    w64, terms = GC.words(mask, closs, ll, aloss, GC.CONS, GC.LAMDA)
    ratio = np.abs(got - w64[:7]) / np.maximum(GC.words_tolerance(w64, terms)[:7], 1e-300)
    print("words N=%d: error / tolerance" % N, np.round(ratio, 4))
    assert (ratio <= 1.0).all()
    assert got[0] == np.float32(mm) and got[1] == closs[0] and got[3] == closs[1], "mask_mean and the copied words are exact"
    assert got[6] == -ll[-1], "the maximum sits in the last row and is a copy"
    again, _, _ = run_words(N, dev)
    assert np.array_equal(got.view(np.int32), again.view(np.int32)), "two runs give the same bits"
    # the critic's part alone leaves the actor's words alone
    from mobody_amd import ops
    w = torch.full((8,), NAN, device=dev)
    d = lambda x: torch.from_numpy(x).to(dev)
    ops.bosa_stage2_words(N, w, mask_mean=d(np.array([mm], np.float32)), closs=d(closs), cons_coef=GC.CONS)
    torch.cuda.synchronize()
    assert np.array_equal(w[:4].cpu().numpy().view(np.int32), got[:4].view(np.int32)) and bool(torch.isnan(w[4:]).all())


def test_stage2_words_keep_a_nan_and_bump_the_counters(dev):
    N = 257
    _, _, ll, _, _ = GC.words_inputs(N)
    ll = ll.copy()
    ll[100] = np.nan
    ctr = torch.tensor([10, 20, 30, 40, 50], dtype=torch.int64, device=dev)
    got, _, _ = run_words(N, dev, ll=ll, bump=ctr)
    clean, _, _ = run_words(N, dev)
    assert np.isnan(got[[4, 5, 6]]).all() and np.array_equal(got[:4].view(np.int32), clean[:4].view(np.int32))
    assert ctr.tolist() == [13, 21, 31, 41, 50]


# ---- 3. the class ---------------------------------------------------------------------------------------------------------------------
class Writer:
    def __init__(self):
        self.seen = []

    def add_scalar(self, k, v, step):
        self.seen.append((k, v, step))


def run(dev, key, calls, bs=8, between=None, writer=None, **over):
    """Two VAE calls, then `calls` stage-2 calls; between(pol, i) runs before stage-2 call i."""
    extra = {} if key is None else dict(critic_actor_graph=key)
    pol = make(dev, vae_iteration=4, critic_actor=1, rng="device", seed=3, **extra, **over)
    load_scaled(pol)
    src, tar = buffers(dev, rng="device", seed=9)
    for i in range(-2, calls):
        if between is not None and i >= 0:
            between(pol, i)
        pol.train(src, tar, bs, writer, None)
    torch.cuda.synchronize()
    return pol, src, tar


def counts(pol, src, tar):
    return (pol.total_it, pol.critic_optimizer.t, pol.actor_optimizer.t, pol._noise_calls, src._draws, tar._draws)


def words_close(g, e, cfg_over=None):
    from test_bosa_ref import bosa_config
    lg, le = g.stage2_log(), e.stage2_log()
    assert list(lg) == list(le)
    terms = BC.scalar_terms(le, bosa_config())
    for k, v in le.items():
        assert abs(lg[k] - v) <= 1e-5 * abs(v) + 1e-5 * terms[k], (k, lg[k], v)


def first_of_each_kind(calls, update_interval, first_total_it=5):
    """The stage-2 calls that run eagerly with the key set: the first critic call and the first actor call size the buffers and make
    every launch once outside a capture."""
    kinds = ["actor" if (first_total_it + i) % update_interval == 0 else "critic" for i in range(calls)]
    return {kinds.index(k) for k in set(kinds)}, kinds


@pytest.mark.parametrize("bs,ui", [(8, 2), (33, 3)])
def test_replayed_stage_two_has_the_bits_of_the_eager_one(bs, ui, dev):
    calls = 10
    g, gs, gt = run(dev, 1, calls, bs, update_interval=ui)
    e, es, et = run(dev, 0, calls, bs, update_interval=ui)
    assert differing(nets_state(g), nets_state(e), skip=("scalars",)) == [], "a replayed run differs from the eager one"
    assert counts(g, gs, gt) == counts(e, es, et) and g.total_it == 4 + calls
    words_close(g, e)
    eager, kinds = first_of_each_kind(calls, ui)
    assert len(eager) == 2 and g.stage2_replays == calls - len(eager) and g.stage2_captures == {"critic": 1, "actor": 1}
    assert e.stage2_replays == 0 and e.stage2_captures == {"critic": 0, "actor": 0} and e._s2_graphs == {}
    assert g._graph is None and e._graph is None
    fresh = make(dev, vae_iteration=4, critic_actor=1, rng="device", seed=3)
    assert "actor" in differing(nets_state(fresh), nets_state(g)), "the run trained"


def test_calls_that_move_the_counts_between_replays(dev):
    """A dyna_log_likelihood call between two replays, and an eager call forced by a writer on a logging step (total_it is set so that the
    seventh call logs and the eighth is on the health cadence): the run goes on with the eager run's bits and without a recapture."""
    calls = 12
    probe = {}

    def between(pol, i):
        if i == 4:
            b = tuple(torch.zeros(5, w, device=dev) for w in (17, 6, 17))
            probe[pol] = pol.dyna_log_likelihood(*b).clone()
        if i == 6:
            pol.total_it = 4999
    wg, we = Writer(), Writer()
    g, gs, gt = run(dev, 1, calls, between=between, writer=wg)
    e, es, et = run(dev, 0, calls, between=between, writer=we)
    assert bits_equal(probe[g], probe[e])
    assert differing(nets_state(g), nets_state(e), skip=("scalars",)) == []
    assert counts(g, gs, gt) == counts(e, es, et) and g.total_it == 5005
    words_close(g, e)
    assert [k for k, _, _ in wg.seen] == [k for k, _, _ in we.seen] and len(wg.seen) == 8 and {s for _, _, s in wg.seen} == {5000}
    # eager: calls 0 and 1 (the first of each kind), call 6 (it logs) and call 7 (total_it 5000: the health cadence)
    assert g.stage2_replays == calls - 4 and g.stage2_captures == {"critic": 1, "actor": 1}


def test_a_checkpoint_resumes_into_replays_bit_for_bit(dev, tmp_path):
    g, gs, gt = run(dev, 1, 6)
    e, es, et = run(dev, 0, 6)
    prefix = str(tmp_path / "model")
    g.save(prefix)
    assert len(os.listdir(tmp_path)) == 13
    fresh = make(dev, vae_iteration=4, critic_actor=1, rng="device", seed=3, critic_actor_graph=1)
    fresh.load(prefix)
    g.load(prefix)
    fresh.total_it, fresh._noise_calls = g.total_it, g._noise_calls
    fs, ft = buffers(dev, rng="device", seed=9)
    fs._draws, ft._draws = gs._draws, gt._draws
    for _ in range(4):
        for pol, s, t in ((fresh, fs, ft), (g, gs, gt), (e, es, et)):
            pol.train(s, t, 8, None, None)
    torch.cuda.synchronize()
    want = nets_state(e)
    assert differing(nets_state(fresh), want, skip=("scalars",)) == [] and differing(nets_state(g), want, skip=("scalars",)) == []
    assert counts(fresh, fs, ft) == counts(g, gs, gt) == counts(e, es, et)
    words_close(fresh, e)
    # the loaded object's first call of each kind is eager, then it replays; the running one went on replaying its two graphs
    # (load() into the running object rewrites the nets in place: its two graphs stay)
    assert fresh.stage2_replays == 2 and g.stage2_replays == 4 + 4 and g.stage2_captures == {"critic": 1, "actor": 1}
    assert fresh.stage2_captures == {"critic": 1, "actor": 1}


def test_without_the_key_graph_replays_the_vae_stage_only(dev):
    """Today's behaviour, which the key at its default keeps: graph = 1 leaves _graph None in stage 2 and captures nothing there."""
    g, gs, gt = run(dev, None, 4, graph=1)
    e, es, et = run(dev, None, 4, graph=0)
    assert g._graph is None and getattr(g, "_s2_graphs", {}) == {} and getattr(g, "stage2_replays", 0) == 0
    assert differing(nets_state(g), nets_state(e)) == [] and counts(g, gs, gt) == counts(e, es, et)


def test_noise_fn_and_host_rng_run_eagerly_through_the_new_entries(dev):
    """With the key set a call that cannot replay -- a noise hook, or rng other than 'device' -- still goes through the row-wise
    entries: the nets of the torch composition, bit for bit."""
    out = {}
    for key in (1, 0):
        pol = make(dev, vae_iteration=0, critic_actor=1, critic_actor_graph=key)
        load_scaled(pol)
        rng = np.random.default_rng(8)
        pol.noise_fn = lambda kind, shape, rng=rng: rng.standard_normal(shape).astype(np.float32)
        src, tar = buffers(dev)
        np.random.seed(11)
        for _ in range(4):
            pol.train(src, tar, 8, None, None)
        torch.cuda.synchronize()
        out[key] = pol
    assert differing(nets_state(out[1]), nets_state(out[0]), skip=("scalars",)) == [] and out[1].stage2_replays == 0
    assert out[1]._noise_calls == out[0]._noise_calls == 4
    words_close(out[1], out[0])


# ---- 4. the CLI -----------------------------------------------------------------------------------------------------------------------
def test_cli_replays_stage_two_with_the_key(tmp_path, monkeypatch):
    from mobody_amd import train_mobody as tm
    from mobody_amd.algo.offline_offline.bosa import vae_steps
    monkeypatch.setenv("MOBODY_CONFIG_ROOT", config_tree(tmp_path, vae_iteration=5, batch_size=16))
    n = vae_steps(5)
    pols = {}
    for key in (1, 0):
        out_dir = tmp_path / ("out%d" % key)
        params = dict(graph=1, critic_actor=1, **({"critic_actor_graph": 1} if key else {}))
        argv = ["--policy", "BOSA", "--env", "walker2d-friction", "--shift_level", "2.0", "--mode", "3", "--seed", "1", "--synthetic", "1",
                "--rng", "device", "--src_rows", "300", "--tar_rows", "200", "--save-model", "--eval_freq", "4", "--log_every", "4",
                "--dir", str(out_dir), "--params", json.dumps(params), "--max_step", str(n + 6)]
        pols[key] = tm.main(argv)
        files = sorted({f for _, _, fs in os.walk(out_dir) for f in fs if f.startswith("model_")})
        assert len(files) == 13 and "model__critic_2_optimizer" in files and "model_critic_1_target" in files
    torch.cuda.synchronize()
    g, e = pols[1], pols[0]
    assert g.total_it == e.total_it == 2 * n + 6 and g.stage2_replays == 4 and g.stage2_captures == {"critic": 1, "actor": 1}
    assert differing(nets_state(g), nets_state(e), skip=("scalars",)) == [] and e.stage2_replays == 0
