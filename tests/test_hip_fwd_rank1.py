"""The output layer of a one-output net (twin-Q) in the fused MLP forward as an fma chain (csrc/tile.h narrow_run_one) instead of
16 x 2 v_mfma_f32_16x16x4_f32 of which one result column is kept (narrow_run): every bit has to stay.

Oracle inside the tree: the same net with out_dim = 2 (a second W3 column and bias of other random values) keeps the MFMA
path, and an MFMA output column does not depend on its neighbours -- column 0 of that run must be torch.equal to the
out_dim = 1 run, bias included.  In the f32 mode both are also held, bit for bit, to the NumPy float32 statement of the
layer's order (tests/fwd_rank1_ref.py) applied to the h2 the launch saved.  Inputs are standard normal, so the 256-term sums
round at every step; the CPU tests show that the emulation is order-sensitive on such data (the reversed chain differs in
most rows) and that its fma is correctly rounded.  Row counts sit on both sides of the 16- and 32-row edges of a tile and
run into a third workgroup; the input widths are the four (S + A) of the product's environments, which take both input
loaders.  No tolerance anywhere: a version that is merely close is not wanted."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import fwd_rank1_ref as R
import golden_util as gu
from mobody_amd import ops, packing

ROWS = [1, 15, 16, 17, 31, 32, 33, 65]
SPLITS = {14: (11, 3), 23: (17, 6), 69: (45, 24), 119: (111, 8)}     # in_dim -> (n0, n1): state | action
MODES = ["f32", "f16x2"]
F32 = np.float32


def _params(seed, in_dim, out_dim, w3_scale=1.0, dead_bias=False):
    """nn.Linear-shaped float32 weights; hidden activations of order one, output weights standard normal"""
    rng = np.random.default_rng(seed)
    n = lambda *s: rng.standard_normal(s).astype(F32)
    b1, b2 = F32(0.1) * n(256), F32(0.1) * n(256)
    if dead_bias:                                                     # an all-zero input row then dies in both hidden layers
        b1, b2 = -np.abs(b1), -np.abs(b2)
    return {"network.0.weight": n(256, in_dim) / F32(np.sqrt(in_dim)), "network.0.bias": b1,
            "network.2.weight": n(256, 256) * F32(np.sqrt(2.0 / 256)), "network.2.bias": b2,
            "network.4.weight": n(out_dim, 256) * F32(w3_scale), "network.4.bias": n(out_dim) * F32(w3_scale)}


def _widen(p, seed):
    """the same net with a second output of other random values"""
    rng = np.random.default_rng(seed)
    q = dict(p)
    scale = F32(np.abs(p["network.4.weight"]).max())
    q["network.4.weight"] = np.concatenate([p["network.4.weight"], scale * rng.standard_normal((1, 256)).astype(F32)])
    q["network.4.bias"] = np.concatenate([p["network.4.bias"], scale * rng.standard_normal(1).astype(F32)])
    return q


@functools.lru_cache(maxsize=None)
def _nets(in_dim, members, mode, w3_scale=1.0, dead_bias=False):
    """(member params, one-output blob, its T blob, two-output blob, its T blob)"""
    dev = torch.device("cuda:0")
    one = [_params(100 * in_dim + m, in_dim, 1, w3_scale, dead_bias) for m in range(members)]
    two = [_widen(p, 7000 + 100 * in_dim + m) for m, p in enumerate(one)]
    b1, b2 = packing.pack_mlp(one, in_dim, 1, dev), packing.pack_mlp(two, in_dim, 2, dev)
    if mode == "f32":
        return one, b1, None, b2, None
    return one, b1, ops.mlp_transpose(b1, in_dim, 1, members, precision=mode), b2, ops.mlp_transpose(b2, in_dim, 2, members, precision=mode)


@functools.lru_cache(maxsize=None)
def _inputs(in_dim, rows):
    g = torch.Generator(device="cpu").manual_seed(31 * in_dim + rows)
    n0, n1 = SPLITS[in_dim]
    dev = torch.device("cuda:0")
    return torch.randn(rows, n0, generator=g).to(dev), torch.randn(rows, n1, generator=g).to(dev)


def _run(nets, in_dim, members, mode, s0, s1):
    """column 0 of the one-output launch [members][rows], of the two-output launch, and the h2 the first saved"""
    _, b1, t1, b2, t2 = nets
    out1, _, _, h2 = ops.mlp3_forward(b1, in_dim, 1, members, s0, s1, save=True, blob_T=t1, precision=mode)
    out2 = ops.mlp3_forward(b2, in_dim, 2, members, s0, s1, blob_T=t2, precision=mode)
    torch.cuda.synchronize()
    return out1[:, :, 0].contiguous(), out2[:, :, 0].contiguous(), h2


def _emulated(nets, h2, members):
    h2 = h2.cpu().numpy()
    return np.stack([R.out_layer(h2[m], nets[0][m]["network.4.weight"][0], nets[0][m]["network.4.bias"][0]) for m in range(members)])


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the emulation itself
# ---------------------------------------------------------------------------------------------------------------------
def test_emulated_fma_is_correctly_rounded():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(3000).astype(F32), rng.standard_normal(3000).astype(F32)
    c = (rng.standard_normal(3000) * np.ldexp(1.0, rng.integers(-20, 21, 3000))).astype(F32)
    c[:500] = -(a[:500].astype(np.float64) * b[:500].astype(np.float64)).astype(F32)      # cancellation: the low product bits decide
    got = R.fma32(a, b, c)
    lo, hi = np.nextafter(got, F32(-np.inf)), np.nextafter(got, F32(np.inf))
    for x, y, z, g, l, h in zip(a, b, c, got, lo, hi):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        d = abs(exact - Fraction(float(g)))
        dl, dh = abs(exact - Fraction(float(l))), abs(exact - Fraction(float(h)))
        assert d <= dl and d <= dh, (x, y, z)                          # no float32 is nearer ...
        assert (d < dl and d < dh) or (int(g.view(np.int32)) & 1) == 0, (x, y, z)     # ... and a tie went to even


def test_order_matters_on_these_inputs():
    """On rounded sums of standard-normal products the documented order is distinguishable: the reversed chain changes most
    rows, and so does the other sequential reading of a wave's 64 k (lane quarter outer)."""
    rng = np.random.default_rng(1)
    h2 = np.maximum(rng.standard_normal((65, 256)), 0).astype(F32)
    w, b = rng.standard_normal(256).astype(F32), F32(0.3)
    want = R.out_layer(h2, w, b)
    for other in (R.reversed_order(), R.q_outer_order()):
        assert (R.out_layer(h2, w, b, other) != want).mean() > 0.5
    assert sorted(k for ks in R.K_ORDER for k in ks) == list(range(256))


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("members", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_one_output_equals_mfma_column(mode, members):
    for in_dim in SPLITS:
        nets = _nets(in_dim, members, mode)
        for rows in ROWS:
            s0, s1 = _inputs(in_dim, rows)
            one, two, h2 = _run(nets, in_dim, members, mode, s0, s1)
            what = (mode, members, in_dim, rows)
            assert torch.isfinite(one).all(), what
            assert torch.equal(_bits(one), _bits(two)), what
            if mode == "f32":
                want = _emulated(nets, h2, members)
                assert np.array_equal(one.cpu().numpy().view(np.int32), want.view(np.int32)), what


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_dead_rows_give_the_bias(mode):
    """Rows whose hidden units are all dead: every product is zero, the output is b3 exactly."""
    in_dim, members, rows = 23, 2, 33
    nets = _nets(in_dim, members, mode, 1.0, True)
    s0, s1 = (t.clone() for t in _inputs(in_dim, rows))
    for r in (5, 32):
        s0[r] = 0
        s1[r] = 0
    one, two, h2 = _run(nets, in_dim, members, mode, s0, s1)
    assert torch.equal(_bits(one), _bits(two))
    assert (h2[:, [5, 32]] == 0).all() and (h2[:, 0] != 0).any()
    for m in range(members):
        b3 = float(nets[0][m]["network.4.bias"][0])
        assert one[m, 5].item() == b3 and one[m, 32].item() == b3
        assert (one[m, :5] != b3).all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("exp", [12, -12])
def test_scaled_output_weights(mode, exp):
    in_dim, members, rows = 14, 2, 65
    nets = _nets(in_dim, members, mode, float(2.0 ** exp))
    s0, s1 = _inputs(in_dim, rows)
    one, two, h2 = _run(nets, in_dim, members, mode, s0, s1)
    assert torch.equal(_bits(one), _bits(two))
    if mode == "f32":
        assert np.array_equal(one.cpu().numpy().view(np.int32), _emulated(nets, h2, members).view(np.int32))
        # a power of two moves no rounding: the unit-scale result, scaled
        base = _run(_nets(in_dim, members, mode), in_dim, members, mode, s0, s1)[0]
        assert torch.equal(one, base * float(2.0 ** exp))


@pytest.mark.gpu
def test_merged_critic_launch_q_and_qt(monkeypatch):
    """mobody_critic with `gather` at (17, 6), N = 33 (the merged forward launch, csrc/critic_fwd_bf.hip): the q and qt it leaves
    in the workspace are the plain forward's of the rows it gathered."""
    monkeypatch.setenv("MOBODY_MFMA", "f16x2")
    from mobody_amd import engine
    S, A, N, mode = 17, 6, 33, "f16x2"
    dev = torch.device("cuda:0")
    pa, pq, _ = gu.policy_params(5, S, A)
    eng = engine.Engine(S, A, pa, pq, dev)
    cfg = gu.policy_cfg(S, A, mfma=mode)
    g = torch.Generator(device="cpu").manual_seed(9)
    store = torch.randn(500, ops.ring_pitch(S, A), generator=g).to(dev)
    ring, size = ops.RingView(store, S, A), torch.tensor([0, 500], dtype=torch.int64, device=dev)
    dims, hyp = ops.train_dims(S, A, N, N), ops.hyper(cfg)
    batch = tuple(torch.zeros((N, w), device=dev) for w in (S, A, S, 1, 1))
    ws = ops.train_workspace(dims, dev)
    ws.view(torch.int32).fill_(-1)
    st = {k: getattr(eng, k).clone() for k in ("actor", "actor_T", "q", "q_T", "qt", "qt_T", "mq", "vq")}
    before = {k: v.clone() for k, v in st.items()}
    loss = torch.zeros(1, device=dev)
    ctr = torch.tensor([7, 3, 11, 13], dtype=torch.int64, device=dev)  # draw counter | the three words the gather advances
    gather = dict(buffers=[ring], counts=[N], seeds=[101], call_offsets=[1], counter=ctr[0:1], sizes=[size[1:2]],
                  bump=(ctr[1:2], ctr[2:3], ctr[3:4]))
    ops.critic_update(dims, hyp, st["actor"], st["q"], st["q_T"], st["qt"], batch, st["mq"], st["vq"], 0, cfg["critic_lr"], loss, ws,
                      t_dev=ctr[1:2], policy_forward=True, actor_blob_T=st["actor_T"], qtarg_blob_T=st["qt_T"], gather=gather)
    torch.cuda.synchronize()
    state, action, next_state = batch[0], batch[1], batch[2]
    r4 = lambda n: (n + 3) & ~3                                        # csrc/train.hip carve: pi | pin | qt [2][N] | q [2][N], pieces of 4 floats
    o_qt = 2 * r4(N * A)
    qt_ws, q_ws = ws[o_qt:o_qt + 2 * N].view(2, N), ws[o_qt + r4(2 * N):o_qt + r4(2 * N) + 2 * N].view(2, N)
    q = ops.mlp3_forward(before["q"], S + A, 1, 2, state, action, blob_T=before["q_T"], precision=mode)[:, :, 0]
    pin = ops.mlp3_forward(before["actor"], S, A, 1, next_state, out_mode=1, max_action=cfg["max_action"], blob_T=before["actor_T"],
                           precision=mode)[0]
    qt = ops.mlp3_forward(before["qt"], S + A, 1, 2, next_state, pin, blob_T=before["qt_T"], precision=mode)[:, :, 0]
    assert torch.isfinite(q).all() and torch.isfinite(qt).all()
    assert torch.equal(_bits(q_ws), _bits(q))
    assert torch.equal(_bits(qt_ws), _bits(qt))
